"""GPU: temperature sampling on chip and Whisper's temperature fallback (wcb_op_lm_head_sample, wcb_generate_sampled,
wcb_decode_enable_sampling; generate(temperature=..., seed=...), decode_begin(temperature=...)).

The sampled token of a step is argmax_v x[v], x[v] = score[v] / T + g(seed of the clip, step, v), score = logit +
bias boost (EOS masked while min_new_tokens holds), g the Gumbel noise of csrc/sample.h. The reference of every test
is that expression in float64, from the logits the device itself returned and the numpy restatement of the noise in
tests/test_abi_sampling.py (checked there against Philox's known answers and the library's host function).

The margin rule. The device computes x in f32 (one fma of an f32 score and an f32 g), the reference in f64: they may
order two candidates differently only when the candidates are closer than the f32 error of x, a few 1e-7·|x|. A row is
compared when the reference's top-two gap exceeds 1e-4·max(1, |x_top|) and counted as skipped otherwise; the skipped
share is bounded (1 % of the op rows, one row of the step-wise test).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.bias_ref import AhoCorasick  # noqa: E402
from test_abi_sampling import noise64  # noqa: E402
from test_gpu_logprobs import (DT, logprob_tol, logsumexp64, lm_head_inputs, lse_bound, mel_batch, model,  # noqa: E402
                               case as lp_case)
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.model import clip_seeds, compression_ratio  # noqa: E402

U64P = C.POINTER(C.c_uint64)
ROWS = {"checked": 0, "skipped": 0}       # the op test's rows over its whole parametrisation
STEP_ROWS = {"checked": 0, "skipped": 0}  # the step-wise test's


def inv_t32(T):
    return float(np.float32(1.0) / np.float32(T))


def reference_sample(scores, T, seeds, step):
    """(token, x_top, decided) per row: argmax of scores64 · inv_T + g64 and whether its margin decides it."""
    scores = np.asarray(scores, dtype=np.float64)
    M, V = scores.shape
    x = np.stack([scores[r] * inv_t32(T) + noise64(int(seeds[r]), step, np.arange(V)) for r in range(M)])
    x[np.isneginf(scores)] = -np.inf
    tok = x.argmax(axis=1)
    top = x[np.arange(M), tok]
    rest = x.copy()
    rest[np.arange(M), tok] = -np.inf
    gap = top - rest.max(axis=1)
    return tok, top, gap > 1e-4 * np.maximum(1.0, np.abs(top))


# ------------------------------------------------------------------------------------------------ 1. the kernel
def lm_head_sample(dt, A, Wt, walkers, T, seeds, step):
    lib = _lib.load()
    M, K = A.shape
    V = Wt.shape[0]
    logits = torch.empty(M, V, device="cuda", dtype=torch.float32)
    lse = torch.empty(M, device="cuda", dtype=torch.float32)
    ids = torch.empty(M, device="cuda", dtype=torch.int32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    _lib.check(lib.wcb_op_lm_head_sample(DT[dt][1], A.data_ptr(), Wt.data_ptr(), M, V, K, walkers, float(T),
                                         seeds.ctypes.data_as(U64P), step, logits.data_ptr(), V, lse.data_ptr(),
                                         ids.data_ptr(), torch.cuda.current_stream().cuda_stream),
               None, "wcb_op_lm_head_sample")
    torch.cuda.synchronize()
    return logits.cpu().numpy(), lse.cpu().numpy(), ids.cpu().numpy().astype(np.int64)


def sample_inputs(dt, kind, M, K, V):
    """lm_head_inputs; the flat kind rescaled to unit-variance logits (A ~ N(0, 1), W ~ N(0, 1 / K))"""
    A, Wt = lm_head_inputs(dt, kind, M, K, V)
    if kind == "flat":
        Wt = (Wt.float() * (1e3 * K ** 0.5)).to(DT[dt][0])
    return A, Wt


def sample_case(dt, kind, M, K, V, walkers, T, step):
    A, Wt = sample_inputs(dt, kind, M, K, V)
    # every case draws with seeds of its own, so the rows of the parametrisation are independent draws
    seeds = clip_seeds(1000 + K + V + 131 * step + 7919 * walkers + int(1000 * T) + (0 if kind == "flat" else 500000), 0, M)
    logits, lse, ids = lm_head_sample(dt, A, Wt, walkers, T, seeds, step)
    a64, w64 = A.double().cpu().numpy(), Wt.double().cpu().numpy()
    ref = a64 @ w64.T
    scale = np.abs(a64) @ np.abs(w64).T + 1.0
    err = (np.abs(logits - ref) / scale).max()   # test_lm_head_lse_op's bounds on the logits and the lse
    assert err < 1e-5, (dt, kind, M, K, V, walkers, err)
    lse64 = logsumexp64(logits)
    assert (np.abs(lse.astype(np.float64) - lse64) <= lse_bound(lse64)).all(), (dt, kind, M, K, V, walkers)
    tok, top, decided = reference_sample(logits, T, seeds, step)
    ROWS["checked"] += int(decided.sum())
    ROWS["skipped"] += int((~decided).sum())
    assert ((ids >= 0) & (ids < V)).all()
    assert np.array_equal(ids[decided], tok[decided]), (dt, kind, M, K, V, walkers, T, step, ids, tok, decided)
    return ids, logits


@pytest.mark.parametrize("K,V", [(64, 649), (384, 649), (32, 649)])   # K = 32: the skinny kernel
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_lm_head_sample_op(dt, K, V):
    moved = []
    for kind in ("flat", "rising"):
        for M in (3, 17):
            for walkers in (128, 1024):
                for T in (0.2, 1.0):
                    for step in (0, 5):
                        ids, logits = sample_case(dt, kind, M, K, V, walkers, T, step)
                        if kind == "flat" and T == 1.0:
                            moved.append((ids != logits.argmax(axis=1)).mean())
    print(f"sample op {dt} K={K} V={V}: rows differing from the argmax at T = 1 (flat): {np.mean(moved):.2f}; "
          f"rows so far {ROWS}")
    assert np.mean(moved) > 0.5   # sampling at T = 1 over unit-variance logits is not the argmax


def test_lm_head_sample_op_full_vocabulary():
    ids, logits = sample_case("bf16", "flat", 17, 64, 51865, 256, 1.0, 5)
    assert (ids != logits.argmax(axis=1)).mean() > 0.5


def test_lm_head_sample_skipped_rows_are_rare():
    """over the whole parametrisation above at most 1 % of the rows fall under the margin rule. Which rows do is
    decided by the reference alone, never by the device. The restatement on the CPU (float64 logits of the same
    inputs, 40 seed sets) leaves out 0.08 % of the flat rows and, of the ramp's rows — neighbouring columns 0.28
    apart at |x_top| near 100, 1.4 apart near 500 at T = 0.2, against margins of 0.01 and 0.05 — 0.9 % at T = 1 and
    2.1 % at T = 0.2: 0.8 % of all rows."""
    print(f"sample op rows: {ROWS}")
    assert ROWS["skipped"] <= 0.01 * (ROWS["checked"] + ROWS["skipped"])


# ------------------------------------------------------------------------------------------------ 2. distribution
def chi2_quantile(df, p_tail=1e-4):
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - p_tail, df))
    except ImportError:   # Wilson-Hilferty; z = the normal 1 - 1e-4 quantile
        z = 3.7190164854556804
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3


def test_sampled_tokens_follow_the_tempered_softmax():
    V, K, R, T = 41, 64, 64, 0.7   # 64 rows x 64 steps = 4,096 draws; V ends mid-tile
    w = 1.0 + (np.arange(V) % 7)   # target probabilities 1..7 / 161: the smallest expected count is 25
    target = T * np.log(w / w.sum())
    a = torch.randn(K, generator=torch.Generator().manual_seed(3))
    A = a[None].repeat(R, 1).contiguous().cuda()
    Wt = (torch.from_numpy(target).float()[:, None] * (a / (a * a).sum())[None]).contiguous().cuda()
    seeds = clip_seeds(2024, 0, R)
    counts, ref_counts = np.zeros(V), np.zeros(V)
    logits = None
    for step in range(64):
        logits, _, ids = lm_head_sample("f32", A, Wt, 128, T, seeds, step)
        counts += np.bincount(ids, minlength=V)
        tok, _, _ = reference_sample(logits, T, seeds, step)
        ref_counts += np.bincount(tok, minlength=V)
    z = logits[0].astype(np.float64) / T
    p = np.exp(z - z.max())
    p /= p.sum()
    expect = p * R * 64
    assert expect.min() >= 5, expect.min()
    q = chi2_quantile(V - 1)
    chi_ref = ((ref_counts - expect) ** 2 / expect).sum()
    chi_dev = ((counts - expect) ** 2 / expect).sum()
    print(f"chi2 at {V - 1} degrees of freedom: restatement {chi_ref:.1f}, device {chi_dev:.1f}, bound {q:.1f}")
    assert chi_ref < q, (chi_ref, q)   # the restatement's own draws first
    assert chi_dev < q, (chi_dev, q)


# --------------------------------------------------------------------------- 3. step-wise against the step's logits
B = 3
T_STEP, SEED_STEP, N_STEP = 0.8, 77, 6
PROMPT = [400, 500, 600]
MODELS = [("f32", "micro"), ("bf16", "tiny"), ("f16", "tiny")]
_STEP = {}


VARIANTS = ["none", "shared", "per_clip", "shared_strong", "per_clip_strong"]


def bias_kw(variant):
    """no boost, a shared list and per-clip lists at lambda = 2, and the two at lambda = 12: there the boost
    outweighs the noise, the rows walk into the phrases, and the finalize's re-scoring of trans(s) and of the
    clip's root children decides the draw"""
    c = lp_case()
    lam = 12.0 if variant.endswith("_strong") else 2.0
    if variant.startswith("shared"):
        return dict(bias_list=c["shared"], bias_boost=lam), [c["shared"]] * B, lam
    if variant.startswith("per_clip"):
        return dict(bias_lists=c["lists"], bias_boost=lam), c["lists"], lam
    return {}, [[]] * B, 0.0


def stepwise(dtype, size, variant, prompt=None):
    """6 sampled steps of the step-wise decoder, every step checked against its own logits; cached: (ids [B, 6],
    log-probs [B, 6]) for the generate() comparison."""
    key = (dtype, size, variant, tuple(prompt or ()))
    if key in _STEP:
        return _STEP[key]
    m = model(dtype, size)
    lib = _lib.load()
    V, eos = m.dims.vocab, m.dims.eos_token_id
    ld = (V + 127) // 128 * 128
    kw, lists, lam = bias_kw(variant)
    acs = [AhoCorasick(L, m.word_start) for L in lists]
    seeds = clip_seeds(SEED_STEP, 0, B)
    dec = m.decode_begin(m.encode(mel_batch(B)), min_new_tokens=N_STEP, logprobs=True, temperature=T_STEP, seed=SEED_STEP,
                         prompt_ids=prompt, **kw)
    try:
        state, live = [0] * B, [True] * B
        toks, want, tol = [], [], []
        buf = torch.empty(B, ld, dtype=torch.float32, device=m.device)
        for t in range(N_STEP):
            ids, sc = dec.step()
            _lib.check(lib.wcb_debug_copy(m._h, b"step_logits", buf.data_ptr(), buf.numel() * 4, -1), m._h, "wcb_debug_copy")
            logits = buf[:, :V].cpu().numpy()
            tok = ids.cpu().numpy().astype(np.int64)
            scores = np.stack([acs[b].boost_row(logits[b], state[b], lam) if lam else logits[b] for b in range(B)])
            scores = scores.astype(np.float32).copy()
            scores[:, eos] = -np.inf   # min_new_tokens: EOS cannot be drawn — it still counts in the lse
            ref, top, decided = reference_sample(scores, T_STEP, seeds, t)
            for b in range(B):
                if live[b] and decided[b]:
                    STEP_ROWS["checked"] += 1
                    assert tok[b] == ref[b], (dtype, size, variant, t, b, tok[b], ref[b])
                    # the step's score is the winner's perturbed value
                    assert abs(float(sc[b]) - top[b]) <= 1e-4 * max(1.0, abs(top[b])), (float(sc[b]), top[b])
                elif live[b]:
                    STEP_ROWS["skipped"] += 1
                    live[b] = False   # a row that may have left the reference's path is not checked further
                state[b] = acs[b].delta(state[b], int(tok[b]))
            lse64 = logsumexp64(logits)
            chosen = logits[np.arange(B), tok]
            toks.append(tok)
            want.append(chosen.astype(np.float64) - lse64)
            tol.append(logprob_tol(chosen, lse64))
        lp = dec.logprobs().cpu().numpy()
        assert lp.shape == (B, N_STEP)
        err = np.abs(lp.astype(np.float64) - np.stack(want, axis=1))
        assert (err <= np.stack(tol, axis=1)).all(), (err.max(), np.stack(tol, axis=1).min())
    finally:
        dec.close()
    _STEP[key] = (np.stack(toks, axis=1), lp)
    return _STEP[key]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype,size", MODELS)
def test_stepwise_samples_match_the_steps_logits(dtype, size, variant):
    ids, _ = stepwise(dtype, size, variant)
    assert ids.shape == (B, N_STEP)
    if variant == "shared_strong":   # the strong boost does pull the rows into the list's phrases
        first = {p[0] for p in lp_case()["shared"]}
        assert all(int(t) in first for t in ids[:, 0]), ids[:, 0]
    print(f"step-wise rows: {STEP_ROWS}")
    assert STEP_ROWS["skipped"] <= 1   # of the whole test


# ------------------------------------------------------------------------------------ 4. generate() equals step-wise
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype,size", MODELS)
def test_generate_equals_stepwise(dtype, size, variant):
    m = model(dtype, size)
    x = mel_batch(B).to(m.device)
    kw, _, _ = bias_kw(variant)
    kw = dict(kw, max_length=N_STEP, min_new_tokens=N_STEP, temperature=T_STEP, seed=SEED_STEP, output_logprobs=True)
    for prompt in (None, PROMPT):
        ids, lp = stepwise(dtype, size, variant, prompt)
        P = 1 + (len(prompt) if prompt else 0)
        for use_graph in (True, False):
            out = m.generate(x, use_graph=use_graph, prompt_ids=prompt, **kw)
            assert np.array_equal(out.sequences[:, P:].cpu().numpy(), ids), (dtype, size, variant, prompt, use_graph)
            assert np.array_equal(out.token_logprobs.cpu().numpy(), lp), (dtype, size, variant, prompt, use_graph)
        # explicit per-clip seeds are the int seed's expansion
        out = m.generate(x, prompt_ids=prompt, **dict(kw, seed=[int(s) for s in clip_seeds(SEED_STEP, 0, B)]))
        assert np.array_equal(out.sequences[:, P:].cpu().numpy(), ids)
        # without log-probs: the same ids (the sampled decode's other graph)
        plain = m.generate(x, prompt_ids=prompt, return_dict_in_generate=True, **dict(kw, output_logprobs=False))
        assert np.array_equal(plain.sequences[:, P:].cpu().numpy(), ids)
        # block=False: device views valid after synchronize(); the seeds array is the call's own temporary
        outs = [m.generate(x, block=False, prompt_ids=prompt, **kw) for _ in range(3)]
        m.synchronize()
        for o in outs:
            assert np.array_equal(o.sequences.cpu().numpy(), ids) and np.array_equal(o.token_logprobs.cpu().numpy(), lp)


# ------------------------------------------------------------------------------------- 5. determinism and graphs
def test_seeds_decide_the_tokens_and_graphs_are_replayed():
    m = model("f32")
    x = mel_batch(B).to(m.device)
    kw = dict(max_length=10, min_new_tokens=10, return_dict_in_generate=True)
    greedy = [m.generate(x, **kw).sequences for _ in range(2)]   # one capture per decode context
    a = [m.generate(x, temperature=1.0, seed=5, **kw).sequences for _ in range(2)]
    assert torch.equal(a[0], a[1])
    assert not torch.equal(a[0], greedy[0])
    captures = m.debug_counter("graph_captures")
    b = m.generate(x, temperature=1.0, seed=6, **kw).sequences
    c = m.generate(x, temperature=0.4, seed=[11, 12, 13], **kw).sequences
    assert m.debug_counter("graph_captures") == captures   # other seeds, another temperature: the same graphs
    assert not torch.equal(a[0], b) and not torch.equal(b, c)
    again = [m.generate(x, **kw).sequences for _ in range(2)]   # the greedy graphs were not evicted
    assert m.debug_counter("graph_captures") == captures
    assert torch.equal(again[0], greedy[0]) and torch.equal(again[1], greedy[0])
    assert torch.equal(m.generate(x, temperature=1.0, seed=5, **kw).sequences, a[0])
    assert m.debug_counter("graph_captures") == captures


# ----------------------------------------------------------------------------------------------- 6. T = 0 is untouched
@pytest.mark.parametrize("dtype,size", MODELS)
def test_temperature_zero_is_the_greedy_call(dtype, size):
    m = model(dtype, size)
    x = mel_batch(B).to(m.device)
    for lp in (False, True):
        kw = dict(min_new_tokens=4, output_logprobs=lp, return_dict_in_generate=True)
        c0 = m.debug_counter("graph_captures")
        ref = [m.generate(x, max_length=11, **kw) for _ in range(2)]
        c1 = m.debug_counter("graph_captures")
        got = m.generate(x, max_length=11, temperature=0.0, seed=9, **kw)
        assert m.debug_counter("graph_captures") == c1   # the greedy call's own graph
        for _ in range(2):
            m.generate(x, max_length=13, temperature=0.0, seed=9, **kw)
        c2 = m.debug_counter("graph_captures")
        assert c1 - c0 == c2 - c1 > 0   # the same captures for a length not seen before
        assert torch.equal(got.sequences, ref[0].sequences)
        if lp:
            assert torch.equal(got.token_logprobs, ref[0].token_logprobs) and torch.equal(got.avg_logprob, ref[0].avg_logprob)
        assert got.temperatures is None


# --------------------------------------------------------------------------------------------------------- 7. split
def test_more_than_64_sampled_clips_split_invisibly():
    m = model("f32")
    x = mel_batch(70)[:66]
    seeds = [int(s) for s in clip_seeds(31, 0, 66)]
    kw = dict(max_length=6, min_new_tokens=6, temperature=0.9, output_logprobs=True)
    whole = m.generate(x, seed=seeds, **kw)
    a, b = m.generate(x[:64], seed=seeds[:64], **kw), m.generate(x[64:], seed=seeds[64:], **kw)
    assert torch.equal(whole.sequences, torch.cat([a.sequences, b.sequences]))
    assert torch.equal(whole.token_logprobs, torch.cat([a.token_logprobs, b.token_logprobs]))
    by_int = m.generate(x, seed=31, **kw)
    assert torch.equal(by_int.sequences, whole.sequences) and torch.equal(by_int.token_logprobs, whole.token_logprobs)
    assert len({tuple(r) for r in whole.sequences.cpu().numpy().tolist()}) > 33   # the clips draw their own noise


# ------------------------------------------------------------------------------------------------------ 8. fallback
def same_rows(m, out, rows, ref, ref_rows=None):
    """rows of `out` equal rows of `ref` up to the padding of the joined output"""
    ref_rows = rows if ref_rows is None else ref_rows
    w = min(out.sequences.shape[1], ref.sequences.shape[1])
    wl = min(out.token_logprobs.shape[1], ref.token_logprobs.shape[1])
    pad = m.dims.pad_token_id
    return (torch.equal(out.sequences[rows, :w], ref.sequences[ref_rows, :w]) and
            bool((out.sequences[rows, w:] == pad).all()) and bool((ref.sequences[ref_rows, w:] == pad).all()) and
            torch.equal(out.token_logprobs[rows, :wl], ref.token_logprobs[ref_rows, :wl]) and
            bool((out.token_logprobs[rows, wl:] == 0).all()) and bool((ref.token_logprobs[ref_rows, wl:] == 0).all()))


def test_temperature_fallback():
    m = model("f32")
    x = mel_batch(4).to(m.device)
    kw = dict(max_length=12, seed=42)
    greedy = m.generate(x, max_length=12, output_logprobs=True)
    avg = greedy.avg_logprob.cpu().numpy()
    order = np.argsort(avg)
    print(f"fallback: greedy avg_logprob {avg}")
    assert len(set(avg.tolist())) == 4
    same = functools.partial(same_rows, m)

    # every clip passes at T = 0
    out = m.generate(x, temperature=(0.0, 0.5, 1.0), logprob_threshold=-np.inf, **kw)
    assert same(out, [0, 1, 2, 3], greedy) and (out.temperatures == 0).all()
    assert torch.equal(out.avg_logprob, greedy.avg_logprob)
    # no clip ever passes: the last temperature's result stands
    out = m.generate(x, temperature=(0.0, 0.5, 1.0), logprob_threshold=float(avg.max()) + 100.0,
                     compression_ratio_threshold=None, **kw)
    assert (out.temperatures == 1.0).all()
    direct = m.generate(x, max_length=12, temperature=1.0, seed=clip_seeds(42, 0, 4, attempt=2), output_logprobs=True)
    assert same(out, [0, 1, 2, 3], direct) and torch.equal(out.avg_logprob, direct.avg_logprob)
    # a threshold between the second and third smallest: exactly those two clips decode again
    thr = float(avg[order[1]] + avg[order[2]]) / 2
    out = m.generate(x, temperature=(0.0, 0.5, 1.0), logprob_threshold=thr, compression_ratio_threshold=None, **kw)
    low, high = sorted(order[:2].tolist()), sorted(order[2:].tolist())
    temps = out.temperatures.cpu().numpy()
    assert (temps[low] > 0).all() and (temps[high] == 0).all(), temps
    assert same(out, high, greedy)
    assert torch.equal(out.avg_logprob[high], greedy.avg_logprob[high])
    second = m.generate(x[low], max_length=12, temperature=0.5, seed=clip_seeds(42, 0, 4, attempt=1)[low], output_logprobs=True)
    for j, b in enumerate(low):   # attempt 1 of the two clips alone, with the whole batch's seeds
        if temps[b] == 0.5:
            assert same(out, [b], second, [j])
    # the compression ratio alone: clip 0 is forced into one repeated token by its own one-token list. A constant
    # row is the most compressible row of its length (12 tokens of 2 bytes: 24 bytes into zlib's ~13), so its ratio
    # lies above every other clip's; the threshold is set between them, as the log-prob thresholds above are
    tok = 1234
    lists = [[[tok]], [], [], []]
    forced = m.generate(x, max_length=12, bias_lists=lists, bias_boost=50.0, output_logprobs=True)
    ids = forced.sequences[:, 1:].cpu().numpy()
    ratios = [compression_ratio(r, m.dims.vocab, m.dims.eos_token_id) for r in ids]
    print(f"fallback: compression ratios {ratios}")
    assert (ids[0] == tok).all() and ratios[0] > max(ratios[1:])
    out = m.generate(x, temperature=(0.0, 0.5, 1.0), logprob_threshold=None,
                     compression_ratio_threshold=(ratios[0] + max(ratios[1:])) / 2,
                     bias_lists=lists, bias_boost=50.0, **kw)
    assert out.temperatures.cpu().numpy().tolist() == [1.0, 0.0, 0.0, 0.0]
    assert same(out, [1, 2, 3], forced)


# The clips of mel_batch(70)[:66] in the order test_temperature_fallback_above_64_clips decodes them. As generated, the
# widest gap of the greedy avg_logprob has clips 19, 41, 43, 48 and 52 below it, all in the first 64; clip 41 changes
# places with clip 64, so that the second library call of the split holds a failing and a passing clip too.
ORDER_66 = list(range(66))
ORDER_66[41], ORDER_66[64] = 64, 41


def test_temperature_fallback_above_64_clips():
    """66 clips, so every attempt is split at 64 clips, and a threshold that fails some clips of both parts: the
    failing clips of the whole batch decode again together, each with the seed of its place in the whole batch."""
    m = model("f32")
    x = mel_batch(70)[:66][ORDER_66]
    seed = 77
    greedy = m.generate(x, max_length=6, output_logprobs=True)
    avg = greedy.avg_logprob.cpu().numpy().astype(np.float64)
    s = np.sort(avg)
    gaps = s[3:64] - s[2:63]   # gaps[k - 3] = s[k] - s[k - 1]: k clips fail, 66 - k pass, k = 3 .. 63
    k = 3 + int(np.argmax(gaps))
    thr = float(s[k - 1] + s[k]) / 2
    fail = avg < thr
    print(f"fallback above 64 clips: {k} clips fail, gap {gaps.max():.3e}, failing {np.flatnonzero(fail).tolist()}, "
          f"order by avg_logprob {np.argsort(avg).tolist()}")
    assert gaps.max() > 1e-3   # the f32 margin of test_temperature_fallback's thresholds
    assert int(fail.sum()) == k
    for part in (fail[:64], fail[64:]):   # both library calls of the split hold a failing and a passing clip
        assert part.any() and not part.all(), fail
    out = m.generate(x, max_length=6, temperature=(0.0, 0.7), seed=seed, logprob_threshold=thr,
                     compression_ratio_threshold=None)
    temps = out.temperatures.cpu().numpy()
    assert np.array_equal(temps, np.where(fail, np.float32(0.7), np.float32(0.0))), temps
    passing = np.flatnonzero(~fail).tolist()
    assert same_rows(m, out, passing, greedy)
    assert torch.equal(out.avg_logprob[passing], greedy.avg_logprob[passing])
    seeds = clip_seeds(seed, 0, 66, attempt=1)
    for b in np.flatnonzero(fail).tolist():
        solo = m.generate(x[b:b + 1], max_length=6, temperature=0.7, seed=[int(seeds[b])], output_logprobs=True)
        assert same_rows(m, out, [b], solo, [0]), b
        assert torch.equal(out.avg_logprob[b:b + 1], solo.avg_logprob), b


# -------------------------------------------------------------------------------------------------------- 9. errors
def test_sampling_errors():
    m = model("f32")
    lib = _lib.load()
    x = mel_batch(B).to(m.device).contiguous()
    ids = torch.empty(B, 6, dtype=torch.int32, device=m.device)
    steps = C.c_int32(0)
    stream = torch.cuda.current_stream().cuda_stream
    seeds = clip_seeds(1, 0, B)

    def sampled(T, beams=1, sd=seeds):
        cfg = _lib.WcbGenCfg(6, 6, beams, 0.0, 1, 0)
        smp = _lib.WcbSampleCfg(T, sd.ctypes.data_as(U64P) if sd is not None else None)
        return lib.wcb_generate_sampled(m._h, x.data_ptr(), B, C.byref(cfg), C.byref(smp), None, None, None, 1,
                                        ids.data_ptr(), None, C.byref(steps), stream)

    assert sampled(1.0) == 0
    for T in (0.0, -1.0, float("nan"), float("inf")):
        assert sampled(T) == -1, T            # WCB_ERR_ARG
    assert sampled(1.0, sd=None) == -1
    assert sampled(1.0, beams=3) == -4         # WCB_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        m.generate(x, max_length=6, num_beams=2, temperature=0.5)
    with pytest.raises(ValueError):
        m.generate(x, max_length=6, temperature=0.5, seed=[1, 2])
    with pytest.raises(ValueError):
        m.generate(x, max_length=6, temperature=-0.5)
    with pytest.raises(ValueError):
        m.generate(x, max_length=6, num_beams=2, temperature=(0.0, 0.5))
    enc = m.encode(x)
    dec = m.decode_begin(enc)
    try:
        assert lib.wcb_decode_enable_sampling(m._h, dec._st, 0.0, seeds.ctypes.data_as(U64P)) == -1
        dec.step()
        assert lib.wcb_decode_enable_sampling(m._h, dec._st, 1.0, seeds.ctypes.data_as(U64P)) == -2   # WCB_ERR_STATE
    finally:
        dec.close()
    dec = m.decode_begin(enc, num_beams=2)
    try:
        assert lib.wcb_decode_enable_sampling(m._h, dec._st, 1.0, seeds.ctypes.data_as(U64P)) == -4
    finally:
        dec.close()
    with pytest.raises(ValueError):
        m.decode_begin(enc, num_beams=2, temperature=0.5)
