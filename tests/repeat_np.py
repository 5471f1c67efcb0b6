"""The tests' numpy restatement of the greedy decoder's repeat rules: HF's repetition penalty and
no-repeat n-gram ban, their planted and random operation-level cases, and a free-running / teacher-forced decode
against the oracle.

For a decoder row, hist = its live prompt tokens, the start token, the forced tail and every token generated so far.
On the raw f32 logits x, before anything else of the step:
  1. penalty p > 0:  for every distinct v in hist   x[v] = x[v] < 0 ? x[v]·p : x[v] / p   (f32, correctly rounded);
  2. n-gram  n >= 1: with L = len(hist) >= n, for every i in [0, L - n] with hist[i : i+n-1] == hist[L-n+1 : L]:
                     x[hist[i+n-1]] = -inf;
  3. then the boost, the EOS mask, the deny list; tok = argmax, lowest index on ties; every score -inf: EOS.
"""
import numpy as np

F32 = np.float32


def banned_tokens(hist, n):
    hist = [int(t) for t in hist]
    L = len(hist)
    if n < 1 or L < n:
        return []
    tail = hist[L - n + 1:]
    return sorted({hist[i + n - 1] for i in range(L - n + 1) if hist[i:i + n - 1] == tail})


def apply_repeat(x, hist, p, n, dtype=F32):
    """The two rules on a copy of the row `x`, in `dtype` arithmetic (float32: the spec, bit for bit; float64: the
    restatement the random operation-level case compares ids against)."""
    s = np.array(x, dtype=dtype)
    seen = sorted({int(t) for t in hist})
    if seen:
        v = s[seen]
        with np.errstate(invalid="ignore"):
            s[seen] = np.where(v < 0, v * dtype(p), v / dtype(p))
    ban = banned_tokens(hist, n)
    if ban:
        s[ban] = -np.inf
    return s


def choose(x, hist, p, n, eos, dtype=F32):
    """(token, its score, top-two score gap) of one row with lam = 0, no EOS mask"""
    s = apply_repeat(x, hist, p, n, dtype)
    if not np.isfinite(s.max()):
        return eos, -np.inf, np.inf
    tok = int(np.argmax(s))
    top2 = np.partition(s.astype(np.float64), -2)[-2:]
    return tok, float(s[tok]), float(top2[1] - top2[0])


# ---------------------------------------------------------------------------------------- operation-level cases
OP = dict(V=2200, K=64, M=17, eos=600)
PLANTED_CALLS = [(2.0, 3), (0.5, 2), (2.0, 1)]   # (p, n): penalised values of k/8 logits stay exact in every dtype
HIST_LENS = [1, 63, 64, 65, 130]                 # around the finalize's 64-lane stride
EDGE_IDS = [31, 32, 63, 64, 2199]                # bitmap-word and 16-column-tile edges, the last id of the vocabulary
N_KINDS = 9
U = 500                                          # the unseen rival of most rows (never in a history)


def planted_case(p, n, M=OP["M"], V=OP["V"], seed=0):
    """(logits [M][V] float32, histories, expected ids): every logit a multiple of 1/8 below 32 in magnitude (exact
    in bf16, f16 and f32), the background in [-3, 3]; row m plants branch m % N_KINDS at history length
    HIST_LENS[m % 5] (or the branch's minimum). The expected id is derived here from the plant, not from choose()."""
    g = np.random.default_rng(seed + int(8 * p) + 100 * n)
    L = g.integers(-24, 25, size=(M, V)).astype(F32) / 8
    hists, expect = [], []
    pen = lambda x: x * p if x < 0 else x / p   # noqa: E731
    for m in range(M):
        k, r, want = m % N_KINDS, L[m], HIST_LENS[m % len(HIST_LENS)]
        fill = [int(t) for t in g.permutation(np.arange(800, 2000))[:200]]   # distinct filler tokens: no accidental n-gram

        def ending_in(tokens, length):   # distinct fillers, then `tokens`
            return fill[:max(0, length - len(tokens))] + list(tokens)
        if k == 0:      # a seen token that loses to an unseen one only because of the penalty (p > 1)
            s = EDGE_IDS[m % 5]
            r[s], r[U] = 20.0, 12.0
            h = ending_in([s], want)
            e = U if (n == 1 or pen(20.0) < 12.0) else s
        elif k == 1:    # a seen token that still wins after the penalty
            s = EDGE_IDS[(m + 1) % 5]
            r[s], r[U] = 28.0, 12.0
            h = ending_in([s], want)
            e = U if n == 1 else s
        elif k == 2:    # p < 1 lifts a seen token over the unseen best
            s = EDGE_IDS[(m + 2) % 5]
            r[s], r[U] = 8.0, 12.0
            h = ending_in([s], want)
            e = U if (n == 1 or pen(8.0) < 12.0) else s
        elif k == 3:    # a negative seen logit: multiplied, not divided
            s = EDGE_IDS[(m + 3) % 5]
            r[:] = r - 20.0
            r[s], r[U] = -8.0, -12.0
            h = ending_in([s], want)
            e = U if (n == 1 or pen(-8.0) < -12.0) else s
        elif k == 4:    # a seen and an unseen token at equal score: the lower index wins
            s = 2199
            r[s], r[40] = 12.0 * p, 12.0
            h = ending_in([s], want)
            e = 40
        elif k == 5:    # a banned token that is the raw argmax
            t, S = 700, [701 + j for j in range(max(n - 1, 0))]
            r[t], r[U] = 30.0, 12.0
            body = S + [t] + fill[100:103] + S
            h = ending_in(body, max(want, len(body)))
            e = U
        elif k == 6:    # a token banned through its second occurrence only
            t, S = 710, [711 + j for j in range(max(n - 1, 0))]
            r[t], r[U] = 30.0, 12.0
            tail = S + [t] + fill[100:103] + S
            h = [t] + ending_in(tail, max(want - 1, len(tail)))
            e = U
        elif k == 7:    # L = n - 1: no ban applies (n = 1: an empty history is not a row; the token is seen and banned)
            a = 64
            r[a], r[U] = 30.0, 12.0
            h = [a] * max(n - 1, 1)
            e = U if n == 1 else a
        else:           # seen tokens at every edge id: each bit must be honoured
            for s in EDGE_IDS:
                r[s] = 20.0
            r[33] = 12.0
            h = ending_in(EDGE_IDS, max(want, len(EDGE_IDS)))
            e = 33 if (n == 1 or pen(20.0) < 12.0) else 31
        hists.append(h)
        expect.append(e)
    return L, hists, np.asarray(expect)


RANDOM_CASE = dict(calls=6, seed=3)
RANDOM_RULES = [(1.3, 0), (1.0, 2), (1.7, 3), (0.6, 2), (2.5, 1), (0.8, 4)]


def random_case(call, torch_dtype):
    """(A [M][K], W [V][K] torch tensors in the dtype, histories, (p, n)) of call `call`: logits N(0, 2.5^2); the
    histories draw from 40 tokens that include each row's 12 largest logits, so repeats, n-gram matches and
    penalised leaders all occur."""
    import torch
    c, r = OP, RANDOM_CASE
    g = torch.Generator(device="cpu").manual_seed(1000 * r["seed"] + call)
    A = torch.randn(c["M"], c["K"], generator=g)
    A = A / A.norm(dim=1, keepdim=True)
    W = torch.randn(c["V"], c["K"], generator=g) * 2.5
    A, W = A.to(torch_dtype), W.to(torch_dtype)
    logits = (A.double() @ W.double().T).numpy()
    rg = np.random.default_rng(r["seed"] * 77 + call)
    hists = []
    for m in range(c["M"]):
        pool = np.concatenate([np.argsort(logits[m])[-12:], rg.integers(0, c["V"], 28)])
        hists.append([int(t) for t in rg.choice(pool, int(rg.integers(1, 131)))])
    return A, W, hists, RANDOM_RULES[call % len(RANDOM_RULES)]


def logit_tol(ref):
    """tests/test_gpu_kernels.py's bound on a decode-row GEMM with f32 output against float64: 1e-4·|ref| + 2e-4"""
    return 1e-4 * np.abs(ref) + 2e-4


def random_expectation(A, W, hists, p, n, eos=OP["eos"]):
    """float64 logits, the restatement's ids in float64, and which rows are decidable: a row may be skipped when its
    top-two score gap is within twice the score error, the logit bound of logit_tol() at the row's largest |logit|
    scaled by max(p, 1/p) (the penalty multiplies or divides a logit, and its error with it)."""
    logits = (A.double() @ W.double().T).numpy()
    ids, ok = [], []
    for m, h in enumerate(hists):
        tok, _, gap = choose(logits[m], h, p, n, eos, np.float64)
        ids.append(tok)
        ok.append(gap > 2 * max(p, 1 / p) * float(logit_tol(np.abs(logits[m]).max())))
    return logits, np.asarray(ids), np.asarray(ok)


# ------------------------------------------------------------------------------------------------- end to end
def repeat_steps(om, enc, p, n, phrases=None, lam=0.0, ids=None, n_tok=24, min_new=0, prompt=(), suppress=()):
    """One clip against the oracle: teacher-forced along `ids` (the device's row) or, ids None, free-running on the
    rule's own choice; hist = prompt + [start] + generated. Per step (token, its score, the top-two score gap, the
    raw logits row): the rules in float32 on the raw row, then the f32 boost (oracle.bias_ref), the EOS mask while
    under min_new and the deny list."""
    from oracle.bias_ref import AhoCorasick
    ac = AhoCorasick(phrases or [])
    xkv = om.cross_kv(enc)
    cache, state, out = {}, 0, []
    hist = [int(t) for t in prompt] + [om.start]
    h = om.decode_tokens(np.asarray([hist]), 0, cache, xkv)
    for t in range(n_tok):
        row = om.lm_head(h[:, -1])[0]
        sc = apply_repeat(row, hist, p, n)
        if lam != 0.0:
            sc = ac.boost_row(sc, state, lam)
        if t < min_new:
            sc[om.eos] = -np.inf
        if len(suppress):
            sc[list(suppress)] = -np.inf
        best = float(sc.max())
        tok = int(ids[t]) if ids is not None else (int(np.argmax(sc)) if np.isfinite(best) else om.eos)
        top2 = np.partition(sc.astype(np.float64), -2)[-2:]
        out.append((tok, float(sc[tok]), float(top2[1] - top2[0]), row))
        if tok == om.eos:
            break
        hist.append(tok)
        state = ac.delta(state, tok)
        h = om.decode_tokens(np.asarray([[tok]]), len(hist) - 1, cache, xkv)
    return out
