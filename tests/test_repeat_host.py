"""CPU: the repeat rules without a device. wcb_repeat_rules_apply_host — the inline functions of
csrc/reprule.h that the finalize compiles — against the numpy restatement (tests/repeat_np.py) bit for bit, and both
against transformers' RepetitionPenaltyLogitsProcessor + NoRepeatNGramLogitsProcessor chained in HF's order; the
planted and random operation-level cases of the GPU tests checked against their own design; resolve()."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repeat_np as RP  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd import request as RQ  # noqa: E402
from whisper_context_biasing_amd.config import get_dims  # noqa: E402

PS, NS = (0.5, 1.2, 2.0), (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def host(lib, x, hist, p, n):
    s = np.array(x, dtype=np.float32)
    h = np.asarray(hist, dtype=np.int32)
    r = _lib.WcbRepeatRules(p, n)
    rc = lib.wcb_repeat_rules_apply_host(C.byref(r), s.shape[0], h.ctypes.data if len(h) else None, len(h), s.ctypes.data)
    return rc, s


def cases():
    """(scores, history, p, n): 400 random rows at V = 2200 (not a multiple of 32) — short vocabularies of repeated
    tokens, zeros, -inf entries, histories shorter than n — then the named ones."""
    g = np.random.default_rng(11)
    out = []
    for i in range(400):
        V = 2200
        x = (g.standard_normal(V) * 3).astype(np.float32)
        x[g.integers(0, V, 20)] = 0.0
        x[g.integers(0, V, 20)] = -np.inf
        pool = g.integers(0, V, int(g.integers(1, 12)))
        hist = [int(t) for t in g.choice(pool, int(g.integers(0, 40)))]
        out.append((x, hist, PS[i % 3], NS[i % 5]))
    x = np.linspace(-4, 4, 2200).astype(np.float32)
    for p in PS:
        for n in (1, 2, 3, 4):
            out.append((x, [7] * (n - 1), p, n))                       # a history shorter than n: no ban
            out.append((x, [5, 9, 1, 2, 9, 3, 4] + [1, 2][:n - 1], p, n))
        out.append((x, [1, 9, 5, 2, 9, 2], p, 2))                      # 9: once after a 2 (banned), once after a 1 (not)
        out.append((np.zeros(2200, np.float32), [0, 3, 2199], p, 0))   # x == 0 (and -0.0 below)
        out.append((-np.zeros(2200, np.float32), [0, 3, 2199], p, 0))
    return out


def test_host_function_equals_the_restatement_bitwise(lib):
    for x, hist, p, n in cases():
        rc, s = host(lib, x, hist, p, n)
        assert rc == 0
        want = RP.apply_repeat(x, hist, np.float32(p), n)
        assert np.array_equal(s.view(np.uint32), want.view(np.uint32)), (hist, p, n)
    # the occurrence rule, spelled out
    _, s = host(lib, np.ones(16, np.float32), [1, 9, 5, 2, 9, 2], 1.0, 2)
    assert np.isinf(s[9]) and np.isfinite(s[[1, 2, 5]]).all()


def test_host_function_equals_transformers(lib):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    for x, hist, p, n in cases():
        if not hist:
            continue
        ids = torch.tensor([hist], dtype=torch.long)
        sc = torch.from_numpy(np.array(x, dtype=np.float32))[None].clone()
        if p != 1.0:
            sc = lp.RepetitionPenaltyLogitsProcessor(penalty=float(np.float32(p)))(ids, sc)
        if n > 0:
            sc = lp.NoRepeatNGramLogitsProcessor(n)(ids, sc)
        _, s = host(lib, x, hist, p, n)
        assert np.array_equal(s.view(np.uint32), sc[0].numpy().view(np.uint32)), (hist, p, n)


def test_argument_errors(lib):
    x = np.zeros(8, np.float32)
    for p, n in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (1.2, -1)):
        assert host(lib, x, [1], p, n)[0] == -1
    assert host(lib, x, [8], 1.2, 0)[0] == -1 and host(lib, x, [-1], 1.2, 0)[0] == -1   # an id outside the vocabulary
    assert lib.wcb_repeat_rules_apply_host(None, 8, None, 0, x.ctypes.data) == -1
    assert lib.wcb_set_repeat_rules(None, None) == -1


def test_planted_cases_hold_what_they_plant():
    for p, n in RP.PLANTED_CALLS:
        L, hists, expect = RP.planted_case(p, n)
        assert np.array_equal(L * 8, np.round(L * 8)) and np.abs(L).max() < 32
        got = [RP.choose(L[m], hists[m], p, n, RP.OP["eos"])[0] for m in range(len(hists))]
        assert np.array_equal(got, expect), (p, n, got, expect)
        raw = L.argmax(axis=1)
        assert (raw != expect).any() and {len(h) for h in hists} >= ({1, 63, 64, 65, 130} if n > 1 else {1, 63, 64})
        seen = {t for h in hists for t in h}
        assert set(RP.EDGE_IDS) <= seen
        # float32 and float64 agree on every planted row: the values are exact
        assert got == [RP.choose(L[m], hists[m], p, n, RP.OP["eos"], np.float64)[0] for m in range(len(hists))]


def test_random_case_stays_inside_the_skip_cap():
    """the seed of the random operation-level case: the restatement alone leaves at most 10 % of the rows inside the
    logit error, in every dtype"""
    torch = pytest.importorskip("torch")
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        ok, changed = [], []
        for call in range(RP.RANDOM_CASE["calls"]):
            A, W, hists, (p, n) = RP.random_case(call, dt)
            logits, ids, good = RP.random_expectation(A, W, hists, p, n)
            ok.extend(good)
            changed.extend(ids != logits.argmax(axis=1))
        assert 1.0 - np.mean(ok) <= 0.10, (dt, np.mean(ok))
        assert np.mean(changed) >= 0.25, "the rules change the winner of a good share of the rows"


def test_resolve_carries_the_two_arguments_in_rules():
    dims = get_dims("micro")
    cfg = SimpleNamespace(max_length=448, num_beams=1)
    base = RQ.resolve(dims, cfg, 2)
    assert base.rules is None
    assert RQ.resolve(dims, cfg, 2, repetition_penalty=1.0, no_repeat_ngram_size=0).rules is None
    r = RQ.resolve(dims, cfg, 2, repetition_penalty=1.3)
    assert r.rules == RQ.NO_TOKEN_RULES + ((float(np.float32(1.3)), 0),)
    assert RQ.split_rules(r.rules) == (None, (float(np.float32(1.3)), 0))
    r = RQ.resolve(dims, cfg, 2, no_repeat_ngram_size=3, suppress_tokens=[5])
    assert r.rules == ((5,), (), False, -1, (1.0, 3)) and RQ.split_rules(r.rules) == (((5,), (), False, -1), (1.0, 3))
    plain = RQ.resolve(dims, cfg, 2, suppress_tokens=[5])
    assert plain.rules == ((5,), (), False, -1) and RQ.split_rules(plain.rules) == (plain.rules, None)
    # the generation config's values apply when the arguments are not given, and an argument overrides them
    cfg2 = SimpleNamespace(max_length=448, num_beams=1, repetition_penalty=1.5, no_repeat_ngram_size=2)
    assert RQ.split_rules(RQ.resolve(dims, cfg2, 2).rules)[1] == (1.5, 2)
    assert RQ.split_rules(RQ.resolve(dims, cfg2, 2, repetition_penalty=1.0).rules)[1] == (1.0, 2)
    assert RQ.resolve(dims, cfg2, 2, repetition_penalty=1.0, no_repeat_ngram_size=0).rules is None
    # take() keeps them
    assert r.take([1]).rules == r.rules


def test_resolve_refusals():
    dims = get_dims("micro")
    cfg = SimpleNamespace(max_length=448, num_beams=1)
    for kw in (dict(num_beams=2), dict(temperature=0.5), dict(temperature=(0.0, 0.4)), dict(do_sample=True),
               dict(return_timestamps=True)):
        for rep in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2)):
            with pytest.raises(ValueError):
                RQ.resolve(dims, cfg, 2, **kw, **rep)
    for rep in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5)):
        with pytest.raises(ValueError):
            RQ.resolve(dims, cfg, 2, **rep)
