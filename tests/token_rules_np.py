"""The tests' numpy restatement of the greedy decoder's token rules, in float64.

For a row that has generated `gen` after its prompt, with score[v] what greedy compares (logit + boost, EOS
masked while under min_new_tokens):
  1. score[v] = -inf for v in suppress; for v in begin_suppress only when t == 0;
  2. with timestamps on, HF WhisperTimeStampLogitsProcessor.__call__ (_detect_timestamp_from_logprob=True);
  3. tok = argmax, lowest index on ties; every score -inf: EOS.
"""
import numpy as np


class Rules:
    def __init__(self, vocab, eos, suppress=(), begin_suppress=(), timestamps=False, ts0=None, no_ts=None, max_init=None):
        self.vocab, self.eos = int(vocab), int(eos)
        self.suppress, self.begin_suppress = [int(v) for v in suppress], [int(v) for v in begin_suppress]
        self.timestamps = bool(timestamps)
        self.ts0 = int(ts0) if ts0 is not None else self.vocab - 1501
        self.no_ts = int(no_ts) if no_ts is not None else self.ts0 - 1
        self.max_init = None if max_init is None or max_init < 0 else int(max_init)

    def abi(self):
        """(wcb_token_rules, keep-alive) for the library"""
        from whisper_context_biasing_amd import _lib
        return _lib.token_rules(self.suppress, self.begin_suppress, self.timestamps, self.ts0, self.no_ts,
                                -1 if self.max_init is None else self.max_init)


def logsumexp(x):
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0 or not np.isfinite(x.max()):
        return -np.inf
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def apply_rules(r, scores, gen, rule5=True):
    """(masked float64 copy of `scores`, lse of the allowed timestamps, best allowed text score) — the two figures
    of rule 5 taken before it is applied (-inf where a side is empty; both None with timestamps off)."""
    s = np.array(scores, dtype=np.float64)
    gen = [int(g) for g in gen]
    t = len(gen)
    s[r.suppress] = -np.inf
    if t == 0:
        s[r.begin_suppress] = -np.inf
    if not r.timestamps:
        return s, None, None
    ts0 = r.ts0
    s[r.no_ts] = -np.inf
    last = t >= 1 and gen[-1] >= ts0
    pen = t < 2 or gen[-2] >= ts0
    if last and pen:
        s[ts0:] = -np.inf
    if last and not pen:
        s[:r.eos] = -np.inf
    stamps = [g for g in gen if g >= ts0]
    if stamps:
        L = stamps[-1]
        s[ts0:(L if (last and not pen) else L + 1)] = -np.inf
    if t == 0:
        s[:ts0] = -np.inf
        if r.max_init is not None:
            s[ts0 + r.max_init + 1:] = -np.inf
    lse_ts, max_text = logsumexp(s[ts0:]), float(s[:ts0].max())
    if rule5 and lse_ts > max_text:
        s[:ts0] = -np.inf
    return s, lse_ts, max_text


def choose(r, scores, gen):
    """(token, lse_ts, max_text) of the rule applied to one row"""
    s, lse_ts, max_text = apply_rules(r, scores, gen)
    tok = int(np.argmax(s)) if np.isfinite(s.max()) else r.eos
    return tok, lse_ts, max_text


def grammar_ok(ids, ts0, eos, pad, max_init=None, denied=(), begin_denied=()):
    """The tolerance-free properties of one generated row decoded with timestamps: no denied token, a first
    timestamp within max_init, timestamps never decreasing, the pairing grammar, pad after EOS."""
    ids = [int(v) for v in ids]
    n = ids.index(eos) if eos in ids else len(ids)
    body = ids[:n]
    assert all(v == pad for v in ids[n + 1:]), ("pad follows EOS", ids)
    assert not set(body) & set(denied), ("denied token", ids)
    assert not body or body[0] not in set(begin_denied), ("begin-denied first token", ids)
    assert body, ("the first token is a timestamp, never EOS", ids)
    assert body[0] >= ts0, ("first token is a timestamp", ids)
    if max_init is not None:
        assert body[0] <= ts0 + max_init, ("first timestamp within max_initial", ids)
    stamps = [v for v in body if v >= ts0]
    assert all(a <= b for a, b in zip(stamps, stamps[1:])), ("timestamps never decrease", ids)
    for i, v in enumerate(body):
        last = i >= 1 and body[i - 1] >= ts0
        pen = i < 2 or body[i - 2] >= ts0
        if last and pen:
            assert v < ts0, ("no third timestamp in a row", i, ids)
        if last and not pen:
            assert v >= eos, ("after text and one timestamp: a timestamp (or a special id >= eos)", i, ids)
    return True


# ---------------------------------------------------------------------------------------- operation-level cases
# max |lse − lse64| in f32 spacings at lse that tests/test_gpu_logprobs.py measured for the same lane-strided +
# butterfly merge (2.28), held at 4x: the rows of the random case whose rule-5 margin lies inside it may be skipped
LSE_BOUND_ULPS = 4 * 2.28


def lse_bound(lse64):
    return LSE_BOUND_ULPS * float(np.spacing(np.float32(abs(lse64))))


def op_rules(V, ts0, eos, timestamps=True, max_init=None):
    """the deny lists of the operation-level cases: text ids, two ids inside [eos, ts0), EOS itself at t == 0"""
    return Rules(V, eos, [3, 40, eos + 5, eos + 9], [5, eos], timestamps, ts0, ts0 - 1, max_init)


N_KINDS = 10


def planted_case(M, V, ts0, eos, offset=0, seed=0):
    """(logits [M][V] float32, histories): every value a multiple of 1/8 below 32 in magnitude (exact in bf16, f16
    and f32), row m planted with branch (m + offset) % N_KINDS of the rule. Text ids lie in [-3, 3], timestamps at
    -30 (their 1501-way logsumexp is -22.7: invisible beside a planted value)."""
    g = np.random.default_rng(seed + 17 * offset + M)
    L = g.integers(-24, 25, size=(M, V)).astype(np.float32) / 8
    L[:, ts0:] = -30.0 + g.integers(0, 2, size=(M, V - ts0)).astype(np.float32) / 8
    gens = []
    for m in range(M):
        k, r = (m + offset) % N_KINDS, L[m]
        if k == 0:      # t == 0: timestamps only; max_initial 50 leaves ts0 + 20, none leaves ts0 + 61
            gen = []
            r[7], r[ts0 + 700], r[ts0 + 20], r[ts0 + 61] = 20.0, 5.0, 3.0, 6.0
        elif k == 1:    # last and penultimate timestamps: text only; denied winners; a tie (lowest index)
            gen = [ts0 + 5, ts0 + 5]
            r[ts0 + 300], r[3], r[40], r[100], r[90] = 20.0, 10.0, 9.0, 6.0, 6.0
        elif k in (2, 3):   # text, then one timestamp: [eos, ts0) and timestamps >= L; rule 5 off (2) / on (3)
            gen = [ts0 + 3, 17, ts0 + 9]
            r[50], r[eos + 5], r[eos + 2], r[eos + 7], r[ts0 + 4] = 12.0, 9.0, 4.0, 4.0, 15.0
            if k == 2:
                r[ts0 + 9] = 3.0
            else:           # three timestamps below the best text score whose sum exceeds it
                r[ts0 + 9], r[ts0 + 10], r[ts0 + 11] = 3.5, 3.5, 3.5
        elif k in (4, 5):   # no timestamp yet: 64 timestamps at 2.0 (logsumexp 6.16); text 6.0 (on) / 8.0 (off)
            gen = [5, 6]
            r[ts0 + 100:ts0 + 164] = 2.0
            r[ts0 + 130] = 2.125
            r[3] = 10.0
            r[200] = 6.0 if k == 4 else 8.0
        elif k == 6:    # L is the last id of the vocabulary, open pair: the one timestamp left against [eos, ts0)
            gen = [ts0 + 1, 9, V - 1]
            r[V - 1], r[eos + 2], r[300] = -2.0, -1.0, 9.0
        elif k == 7:    # L the last id, pair closed, text since: no timestamp is left
            gen = [ts0 + 1, 9, V - 1, V - 1, 7]
            r[V - 1], r[300] = 25.0, 5.0
        elif k == 8:    # a closed pair in mid range: timestamps > L only
            gen = [ts0, 11, ts0 + 50, ts0 + 50, 14]
            r[ts0 + 50], r[ts0 + 51], r[400] = 20.0, 7.0, 6.5
        else:           # t == 1 after the first timestamp: text only; a tie across two tiles and two bitmap words
            gen = [ts0 + 2]
            r[ts0 + 2], r[16], r[48], r[eos] = 20.0, 5.0, 5.0, 4.0
        gens.append(gen)
    return L, gens


def random_history(g, n, ts0, V):
    gen = []
    for _ in range(n):
        u = g.random()
        if u < 0.3:
            gen.append(int(g.integers(ts0, V)))
        elif u < 0.45 and gen and gen[-1] >= ts0:
            gen.append(gen[-1])
        else:
            gen.append(int(g.integers(0, ts0)))
    return gen


RANDOM_CASE = dict(V=2200, ts0=699, eos=600, K=64, M=17, calls=6, seed=5)


def random_case(call, torch_dtype):
    """(A [M][K], W [V][K] torch tensors in the dtype, histories) of call `call` of the random parametrisation: text
    logits N(0, 2.5^2), timestamp logits N(0, 0.5^2), so logsumexp(timestamps) and max(text) both land near 7.5"""
    import torch
    c = RANDOM_CASE
    g = torch.Generator(device="cpu").manual_seed(1000 * c["seed"] + call)
    A = torch.randn(c["M"], c["K"], generator=g)
    A = A / A.norm(dim=1, keepdim=True)
    W = torch.randn(c["V"], c["K"], generator=g)
    W[:c["ts0"]] *= 2.5
    W[c["ts0"]:] *= 0.5
    rg = np.random.default_rng(c["seed"] * 77 + call)
    gens = [random_history(rg, int(rg.integers(0, 8)), c["ts0"], c["V"]) for _ in range(c["M"])]
    return A.to(torch_dtype), W.to(torch_dtype), gens


# ------------------------------------------------------------------------------------------------- end to end
def ruled_steps(om, enc, rules, phrases, lam, ids=None, n=24, min_new=0):
    """One clip against the oracle: teacher-forced along `ids` (the device's row) or, ids None, free-running on the
    rule's own choice. Per step (token, its score, the best allowed score, rule-5 margin or inf, raw logits row):
    scores are the f32 boosted logits (oracle.bias_ref) with the rule applied in float64."""
    from oracle.bias_ref import AhoCorasick
    ac = AhoCorasick(phrases or [])
    xkv = om.cross_kv(enc)
    cache, state, gen, out = {}, 0, [], []
    tok_in = om.start
    for t in range(n):
        h = om.decode_tokens(np.asarray([[tok_in]]), t, cache, xkv)
        row = om.lm_head(h[:, -1])[0]
        sc = ac.boost_row(row, state, lam) if lam != 0.0 else row.copy()
        if t < min_new:
            sc[om.eos] = -np.inf
        s, lse_ts, max_text = apply_rules(rules, sc, gen)
        margin = abs(lse_ts - max_text) if (lse_ts is not None and np.isfinite(lse_ts) and np.isfinite(max_text)) else np.inf
        best = float(s.max())
        tok = int(ids[t]) if ids is not None else (int(np.argmax(s)) if np.isfinite(best) else om.eos)
        # the score the token holds when rule 5 is left open: what a near-tie step is judged by
        out.append((tok, float(s[tok]), best, margin, row))
        if tok == om.eos:
            break
        gen.append(tok)
        state = ac.delta(state, tok)
        tok_in = tok
    return out
