"""GPU: per-utterance bias lists (wcb_bias_batch / wcb_generate_biased / wcb_decode_bias_batch).

Clip b of a batch is boosted with its own phrase list L_b; every decoder row of clip b must be scored
exactly as oracle/bias_ref.py scores it for AhoCorasick(L_b) — so row b of the batched decode equals the
oracle's decode of clip b alone with L_b (f32 mode, token-exact), a clip with an empty list decodes as
plain greedy / plain beam search, and the result differs from the union-of-the-batch decode the shared
automaton gives. Micro model, seed 0, "diverse", 3 clips.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_np as W  # noqa: E402
from oracle.beam_np import generate_beam  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list, synth_word_start  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

B = 3
_CASE, _MODELS, _REF = {}, {}, {}


def case():
    if not _CASE:
        dims = get_dims("micro")
        om = W.OracleModel.from_dims(dims, make_weights(dims, seed=0, recipe="diverse"))
        mel = W.log_mel(synth_batch(B), dims.n_mel)
        enc = om.encode(mel)
        plain = om.generate(mel, enc=enc, max_length=16, min_new_tokens=16)
        eot = dims.eos_token_id
        lists = [synth_bias_list(200, eot=eot, seed=7) + [list(map(int, plain[0, 2:5]))],
                 synth_bias_list(200, eot=eot, seed=8) + [list(map(int, plain[1, 1:3])) + [7, 8]],
                 []]
        _CASE.update(dims=dims, om=om, mel=mel, enc=enc, plain=plain, lists=lists, x=torch.from_numpy(mel))
    c = _CASE
    return c["dims"], c["om"], c["mel"], c["enc"], c["plain"], c["lists"], c["x"]


def model(dtype="f32", **options):
    key = (dtype, tuple(sorted(options.items())))
    if key not in _MODELS:
        dims = get_dims("micro")
        _MODELS[key] = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0, recipe="diverse"), dtype=dtype,
                                                 options=options or None)
    return _MODELS[key]


def greedy_ref(lists, lam, gate, n=16):
    """[B, n]: the oracle's greedy decode of every clip alone with its own list (computed once per case)."""
    dims, om, mel, enc, *_ = case()
    key = ("g", tuple(tuple(map(tuple, L)) for L in lists), lam, gate, n)
    if key not in _REF:
        ws = synth_word_start(dims.eos_token_id, dims.vocab) if gate else None
        rows = [om.generate(mel[b:b + 1], enc=enc[b:b + 1], max_length=n, min_new_tokens=n, bias=lists[b],
                            bias_boost=lam, word_start=ws) for b in range(B)]
        _REF[key] = np.concatenate(rows, 0)
    return _REF[key]


def beam_ref(lists, lam=2.0, n=10):
    """per clip: the oracle's beam-3 result of the clip alone with its own list"""
    dims, om, mel, enc, *_ = case()
    key = ("b", tuple(tuple(map(tuple, L)) for L in lists), lam, n)
    if key not in _REF:
        _REF[key] = [generate_beam(om, enc=enc[b:b + 1], num_beams=3, max_length=n, min_new_tokens=n, bias=lists[b],
                                   bias_boost=lam)[0] for b in range(B)]
    return _REF[key]


def rows_match(got, refs, pad):
    """got [B, W] (batch output, padded to its longest row) against per-clip rows of their own widths"""
    for b, r in enumerate(refs):
        w = len(r)
        if got.shape[1] < w or not np.array_equal(got[b, :w], r) or not (got[b, w:] == pad).all():
            return False
    return True


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("lam", [2.0, 8.0])
def test_greedy_per_utterance_matches_oracle_f32(lam, gate, use_graph):
    dims, om, mel, enc, plain, lists, x = case()
    m = model("f32")
    ws = synth_word_start(dims.eos_token_id, dims.vocab) if gate else None
    m.set_word_start(ws)
    try:
        kw = dict(max_length=16, min_new_tokens=16, bias_boost=lam, use_graph=use_graph)
        got = m.generate(x, bias_lists=lists, **kw).cpu().numpy()
        union = m.generate(x, bias_list=[p for L in lists for p in L], **kw).cpu().numpy()
    finally:
        m.set_word_start(None)
    ref = greedy_ref(lists, lam, gate)
    assert np.array_equal(got, ref), (got, ref)
    assert np.array_equal(got[2], plain[2])                       # an empty list: plain greedy
    assert not np.array_equal(got[1], union[1]) and not np.array_equal(got[2], union[2])


@pytest.mark.parametrize("chunks", [0, 1])
def test_beam3_per_utterance_matches_oracle_f32(chunks):
    dims, om, mel, enc, plain, lists, x = case()
    m = model("f32", beam_chunks=chunks) if chunks else model("f32")
    kw = dict(max_length=10, min_new_tokens=10, num_beams=3, bias_boost=2.0)
    got = m.generate(x, bias_lists=lists, **kw).cpu().numpy()
    refs = beam_ref(lists)
    assert rows_match(got, refs, dims.pad_token_id), (got, refs)
    if not chunks:
        union = m.generate(x, bias_list=[p for L in lists for p in L], **kw).cpu().numpy()
        for b in (1, 2):
            assert not rows_match(union[b:b + 1], refs[b:b + 1], dims.pad_token_id), (b, union, refs)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_same_list_for_every_clip_is_bit_identical_to_shared_path(dtype):
    """The logits are identical and both selections are exact, so the ids must be equal (both LM-head
    epilogues: the lean fused one in bf16, the tiled one in f32)."""
    dims, om, mel, enc, plain, lists, x = case()
    m = model(dtype)
    L = synth_bias_list(200, eot=dims.eos_token_id) + [list(map(int, plain[0, 2:5])), list(map(int, plain[1, 1:3])) + [7, 8]]
    for kw in (dict(max_length=16, min_new_tokens=16), dict(max_length=10, min_new_tokens=10, num_beams=3)):
        shared = m.generate(x, bias_list=L, bias_boost=2.0, **kw)
        per = m.generate(x, bias_lists=[L] * B, bias_boost=2.0, **kw)
        assert torch.equal(shared, per), (kw, shared, per)


def _collate_spans(samples, pad=50256):
    """bias_spans as the reference collator pads them (tests/test_gpu_e2e.py _collate_spans)"""
    L = max(len(sp) for s in samples for sp in s)
    N = max(len(s) for s in samples)
    return torch.tensor([[list(sp) + [pad] * (L - len(sp)) for sp in s] + [[pad] * L] * (N - len(s))
                         for s in samples], dtype=torch.long)


def test_collator_spans_per_utterance():
    dims, om, mel, enc, plain, lists, x = case()
    m = model("f32")
    samples = [[list(map(int, plain[0, 2:5])), [11, 12]], [list(map(int, plain[1, 1:3])) + [7, 8]], [[13, 14, 15]]]
    spans = _collate_spans(samples)
    kw = dict(max_length=16, min_new_tokens=16, bias_boost=2.0)
    per = m.generate(x, bias_spans=spans, per_utterance_bias=True, **kw).cpu().numpy()
    via_lists = m.generate(x, bias_lists=samples, **kw).cpu().numpy()
    assert np.array_equal(per, via_lists) and np.array_equal(per, greedy_ref(samples, 2.0, False))
    zeros = m.generate(x, bias_spans=torch.zeros(B, 1, 1, dtype=torch.long), per_utterance_bias=True, **kw).cpu().numpy()
    assert np.array_equal(zeros, plain)
    union = m.generate(x, bias_spans=spans, **kw).cpu().numpy()             # the default stays the union
    via_union = m.generate(x, bias_list=[s for smp in samples for s in smp], **kw).cpu().numpy()
    assert np.array_equal(union, via_union)


def test_stepwise_per_utterance_equals_generate():
    dims, om, mel, enc, plain, lists, x = case()
    m = model("f32")
    e = m.encode(x)
    n = 16
    ref = m.generate(x, max_length=n, min_new_tokens=n, bias_lists=lists, bias_boost=2.0).cpu().numpy()
    dec = m.decode_begin(e, bias_lists=lists, bias_boost=2.0, min_new_tokens=n)
    # a shared automaton on top of the installed forest is refused, and the state is untouched
    ids = torch.empty(B, dtype=torch.int32, device=m.device)
    sc = torch.empty(B, dtype=torch.float32, device=m.device)
    bl = m.bias_list(lists[0])
    assert m._lib.wcb_decode_step(m._h, dec._st, bl._h, ids.data_ptr(), sc.data_ptr(), None) == -1
    got = torch.stack([dec.step()[0] for _ in range(n)], 1).cpu().numpy()
    dec.close()
    assert np.array_equal(got, ref), (got, ref)
    assert np.array_equal(got, greedy_ref(lists, 2.0, False))
    L = 10
    ref = m.generate(x, max_length=L, min_new_tokens=L, num_beams=3, bias_lists=lists, bias_boost=2.0).cpu().numpy()
    dec = m.decode_begin(e, num_beams=3, max_length=L, bias_lists=lists, bias_boost=2.0, min_new_tokens=L)
    for _ in range(L):
        dec.step()
    got = dec.result().cpu().numpy()
    dec.close()
    assert np.array_equal(got, ref), (got, ref)


def test_new_lists_replay_the_captured_graph():
    """The decode graph reads the forest through the handle's stable buffers: other lists of the same sizes
    replay it (the two decode contexts each captured theirs in the first two calls). And the forest is
    copied at the call: generate() drops its batch object right after an asynchronous call."""
    dims, om, mel, enc, plain, lists, x = case()
    m = model("f32")
    kw = dict(max_length=16, min_new_tokens=16, bias_boost=2.0)
    other = [lists[1], lists[0], []]
    for _ in range(2):
        first = m.generate(x, bias_lists=lists, **kw).cpu().numpy()
    captures = m.debug_counter("graph_captures")
    assert captures > 0
    for _ in range(2):
        second = m.generate(x, bias_lists=other, **kw).cpu().numpy()
    assert m.debug_counter("graph_captures") == captures
    assert np.array_equal(first, greedy_ref(lists, 2.0, False))
    assert np.array_equal(second, greedy_ref(other, 2.0, False))
    out = m.generate(x, bias_lists=lists, block=False, **kw)
    m.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)
    with pytest.raises(_lib.WcbError):
        m.debug_counter("no_such_counter")


def test_argument_errors_and_zero_boost():
    dims, om, mel, enc, plain, lists, x = case()
    m = model("f32")
    kw = dict(max_length=16, min_new_tokens=16)
    with pytest.raises(ValueError):
        m.generate(x, bias_lists=lists[:2], bias_boost=2.0, **kw)
    with pytest.raises(ValueError):
        m.generate(x, bias_lists=[[[1, dims.vocab]], [], []], bias_boost=2.0, **kw)
    # the raw ABI: a batch built for another B, decreasing offsets
    h = _lib.C.c_void_p()
    toks = np.asarray([5, 6, 7], dtype=np.int32)
    poff = np.asarray([0, 2, 3], dtype=np.int32)
    coff = np.asarray([0, 1, 2], dtype=np.int32)
    assert m._lib.wcb_bias_batch_create(m._h, 2, toks.ctypes.data, poff.ctypes.data, coff.ctypes.data, None,
                                        _lib.C.byref(h)) == 0
    assert m._lib.wcb_bias_batch_num_states(h, 0) == 3 and m._lib.wcb_bias_batch_num_states(h, 1) == 2
    assert m._lib.wcb_bias_batch_num_states(h, -1) == 5
    cfg = _lib.WcbGenCfg(16, 16, 1, 2.0, 1, 0)
    out = torch.empty(B, 16, dtype=torch.int32, device=m.device)
    steps = _lib.C.c_int32(0)
    xd = x.to(m.device)
    assert m._lib.wcb_generate_biased(m._h, xd.data_ptr(), B, _lib.C.byref(cfg), h, None, 1, out.data_ptr(),
                                      _lib.C.byref(steps), None) == -1
    m._lib.wcb_bias_batch_destroy(h)
    bad = np.asarray([0, 2, 1], dtype=np.int32)
    h2 = _lib.C.c_void_p()
    assert m._lib.wcb_bias_batch_create(m._h, 2, toks.ctypes.data, bad.ctypes.data, coff.ctypes.data, None,
                                        _lib.C.byref(h2)) == -1
    assert m._lib.wcb_bias_batch_create(m._h, 2, toks.ctypes.data, poff.ctypes.data, bad.ctypes.data, None,
                                        _lib.C.byref(h2)) == -1
    zero = m.generate(x, bias_lists=lists, bias_boost=0.0, **kw)
    assert torch.equal(zero, m.generate(x, **kw))
