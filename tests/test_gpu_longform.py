"""GPU: long-form transcription.

1. wcb_log_mel_long against HF's extractor in long mode (tests/golden/longform_mel.npz) at the front end's 2e-5: both
   clips, 80 and 128 mel bins, the last partial 64-frame block, the frames past the short clip's audio, and a clamp
   that tells the whole-clip maximum from a per-window one.
2. wcb_op_window_cut against numpy, bit-exact, in bf16 / f16 / f32; wcb_encode_windows bit-identical to wcb_encode.
3. The no-speech probability against the step's own logits (the logsumexp bound of tests/test_gpu_logprobs.py) and
   against the oracle; ids bit-identical with the probe on and off.
4. transcribe_long end to end on the micro model, f32: the three fixture clips in one batch against the reference
   class's own long-form output, every clip alone, per-clip bias lists against tests/longform_np.py, the skip rule,
   one bf16 run through the margin gate, the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longform_np as LN  # noqa: E402
from oracle import whisper_np as W  # noqa: E402
from test_gpu_configs import TAU  # noqa: E402
from test_gpu_logprobs import logprob_tol, logsumexp64  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.config import get_dims, no_speech_token_id  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB, _WindowBatch  # noqa: E402
from whisper_context_biasing_amd.prompts import pack_prompts  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch  # noqa: E402

DT = {"bf16": (torch.bfloat16, _lib.WCB_BF16), "f16": (torch.float16, _lib.WCB_F16), "f32": (torch.float32, _lib.WCB_F32)}
MEL_TOL = 2e-5                       # the front end's tolerance against the reference extractor (tests/test_gpu_kernels.py)
LOGPROB_ATOL, LOGPROB_RTOL = 1e-3, 1e-4   # a device log-prob against the oracle's (tests/test_gpu_logprobs.py)
MEL_SLICES, mel_clips = LN.MEL_SLICES, LN.mel_clips
MEL_GOLD = np.load(os.path.join(LN.GOLDEN, "longform_mel.npz"))
E2E = np.load(os.path.join(LN.GOLDEN, "longform_micro_diverse_s0.npz"))


# ------------------------------------------------------------------------------------------- 1. long log-mel
@pytest.mark.parametrize("n_mel,split", [(80, 0), (128, 0), (80, 1)])
def test_long_log_mel(n_mel, split):
    m = WhisperCB(get_dims("micro", n_mel=n_mel), dtype="f32", options={"mel_split": split})   # (no weights: the front end alone)
    clips = mel_clips()
    mel, frames = m.log_mel_long(clips)
    assert tuple(mel.shape) == (2, n_mel, 3337) and frames.tolist() == MEL_GOLD[f"max_frames_{n_mel}"].tolist()
    got = mel.cpu().numpy()
    assert np.isfinite(got).all()
    for i in range(2):
        sl = np.concatenate([got[i][:, s] for s in MEL_SLICES[i]], axis=1)
        err = np.abs(sl - MEL_GOLD[f"mel{n_mel}_clip{i}_slices"]).max()
        st = MEL_GOLD[f"mel{n_mel}_clip{i}_stats"]
        print(f"long log-mel n_mel {n_mel} split {split} clip {i}: slices max err {err:.3g}, max {got[i].max():.6f} / {st[2]:.6f}, "
              f"min {got[i].min():.6f} / {st[3]:.6f}, mean err {abs(got[i].sum(dtype=np.float64) - st[0]) / got[i].size:.3g}")
        assert err < MEL_TOL
        assert abs(got[i].max() - st[2]) < MEL_TOL and abs(got[i].min() - st[3]) < MEL_TOL
        assert abs(got[i].sum(dtype=np.float64) - st[0]) < MEL_TOL * got[i].size
        fw = MEL_GOLD[f"mel{n_mel}_clip{i}_first_window_min_max"]
        assert abs(got[i][:, :3000].min() - fw[0]) < MEL_TOL and abs(got[i][:, :3000].max() - fw[1]) < MEL_TOL
    # MEL_SLICES cover the last partial 64-frame block (3337 = 52 * 64 + 9) and the frames past clip 1's 1250
    assert MEL_SLICES[0][-1].stop == 3337 and MEL_SLICES[1][1].start < 1250 < MEL_SLICES[1][1].stop
    # the clamp is the whole clip's: clip 0's loudest half second lies past its first 30 s, so a per-window maximum
    # would leave the first window's floor far lower (what the 30 s front end gives on those samples alone)
    alone = m.log_mel(torch.from_numpy(clips[0][:480000])).cpu().numpy()[0]
    assert got[0][:, :3000].min() - alone.min() > 0.5, (got[0][:, :3000].min(), alone.min())
    # num_samples: the samples past it read as zero — the padded batch is the same call on an array with explicit lengths
    x = np.zeros((2, len(clips[0])), dtype=np.float32)
    x[0], x[1, :len(clips[1])] = clips[0], clips[1]
    x[1, len(clips[1]):] = 0.3   # (must not be read)
    mel2, frames2 = m.log_mel_long(x, num_samples=[len(clips[0]), len(clips[1])])
    assert torch.equal(mel2, mel) and frames2.tolist() == frames.tolist()
    lib = _lib.load()
    out = torch.empty(1, n_mel, 10, device="cuda")
    pcm = torch.zeros(1, 1600, device="cuda")
    one = np.asarray([1600], dtype=np.int32)
    for nv, n_total, stride, T_ld in ((1601, 1600, 1600, 10), (1600, 1600, 1599, 10), (1600, 1600, 1600, 9), (1600, 640, 1600, 10)):
        one[0] = nv
        assert lib.wcb_log_mel_long(m._h, pcm.data_ptr(), 1, one.ctypes.data, n_total, stride, out.data_ptr(), T_ld, None) == -1


# --------------------------------------------------------------------------------------------- 2. window cut
T, T_LD, N_MEL = 3337, 3344, 80
CUT_SEEKS = [0, 1, 63, 64, 337, 3336]
CUT_ROWS = [(s, min(T - s, 3000)) for s in CUT_SEEKS] + [(0, 3000), (0, 337), (0, 1)]


def window_cut(dt, feats, clip_idx, seek, frames, T_=T):
    lib = _lib.load()
    rows = len(seek)
    xt = torch.full((rows, 3002, feats.shape[1]), 7.0, dtype=DT[dt][0], device="cuda")   # (every element must be written)
    a = [np.ascontiguousarray(np.asarray(v, dtype=np.int32)) for v in (clip_idx, seek, frames)]
    rc = lib.wcb_op_window_cut(DT[dt][1], feats.data_ptr(), feats.shape[0], feats.shape[1], T_, feats.shape[2], rows,
                               a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, xt.data_ptr(), None)
    return rc, xt


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_window_cut(dt):
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(2, N_MEL, T_LD, generator=g)
    feats[:, :, T:] = float("nan")   # the pad columns: nothing past T may be read
    fd = feats.cuda()
    clip_idx = [[1, 0, 1][r % 3] for r in range(len(CUT_ROWS))]   # rows map to clips out of order
    rc, xt = window_cut(dt, fd, clip_idx, [s for s, _ in CUT_ROWS], [n for _, n in CUT_ROWS])
    assert rc == 0
    want = torch.zeros(len(CUT_ROWS), 3002, N_MEL, dtype=DT[dt][0])
    for r, (s, n) in enumerate(CUT_ROWS):
        want[r, 1:1 + n] = feats[clip_idx[r], :, s:s + n].T.to(DT[dt][0])
    got = xt.cpu()
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got, want)
    for r, (s, n) in enumerate(CUT_ROWS):   # (what torch.equal already says, spelled out)
        assert (got[r, 0] == 0).all() and (got[r, 3001] == 0).all() and (got[r, 1 + n:] == 0).all()
    for ci, s, n in ((0, -1, 10), (0, 0, 0), (0, 0, 3001), (0, 338, 3000), (0, 3337, 1), (2, 0, 10), (-1, 0, 10)):
        assert window_cut(dt, fd, [ci], [s], [n])[0] == -1, (ci, s, n)
    assert window_cut(dt, fd, [0], [0], [10], T_=T_LD + 1)[0] == -1   # T > T_ld


_MODELS = {}


def micro(dtype="f32", recipe="diverse"):
    if (dtype, recipe) not in _MODELS:
        c = LN.e2e_case(recipe)
        _MODELS[dtype, recipe] = WhisperCB.from_state_dict(c["dims"], c["sd"], dtype=dtype)
    return _MODELS[dtype, recipe]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_encode_windows_is_encode(dtype):
    m = micro(dtype)
    x = torch.from_numpy(W.log_mel(synth_batch(2), m.dims.n_mel)).cuda()
    ref = m.encode(x)
    assert torch.equal(m.encode_windows(x, [0, 1], [0, 0], [3000, 3000]), ref)
    assert torch.equal(m.encode_windows(x, [1, 0, 1], [0, 0, 0], [3000, 3000, 3000]), ref[[1, 0, 1]])
    with pytest.raises(ValueError):
        m.encode_windows(x, [0], [1], [3000])
    # a short window is the zero-padded window
    pad = x.clone()
    pad[:, :, 500:] = 0.0
    assert torch.equal(m.encode_windows(x, [0, 1], [0, 0], [500, 500]), m.encode(pad))


# ------------------------------------------------------------------------------------------- 3. no-speech
def test_no_speech_probability():
    c = LN.e2e_case()
    m, dims, om = micro(), c["dims"], c["om"]
    B, V, nsp_id = 3, dims.vocab, no_speech_token_id(dims)
    mel = W.log_mel(synth_batch(B), dims.n_mel)
    x = torch.from_numpy(mel).cuda()
    lib = _lib.load()
    ld = (V + 127) // 128 * 128
    kw = dict(return_timestamps=True, max_initial_timestamp=1.0, suppress_tokens=c["suppress"], begin_suppress_tokens=c["begin"])
    with pytest.raises(ValueError):
        m.decode_begin(m.encode(x), no_speech=True, **kw)
    dec = m.decode_begin(m.encode(x), logprobs=True, no_speech=True, **kw)
    try:
        ids0, _ = dec.step()
        buf = torch.empty(B, ld, dtype=torch.float32, device=m.device)
        _lib.check(lib.wcb_debug_copy(m._h, b"step_logits", buf.data_ptr(), buf.numel() * 4, -1), m._h, "wcb_debug_copy")
        dec.step()   # a later step leaves the value alone
        got = dec.no_speech_prob().cpu().numpy().astype(np.float64)
    finally:
        dec.close()
    logits = buf[:, :V].cpu().numpy()
    lse64 = logsumexp64(logits)
    want_log = logits[:, nsp_id].astype(np.float64) - lse64
    # the device: expf(logit - lse) in f32 — the log-prob's own bound, plus the exponential's rounding (2 ulp) and the
    # result's (1 ulp), relative
    rel = logprob_tol(logits[:, nsp_id], lse64) + 3 * 2.0 ** -23
    err = np.abs(got / np.exp(want_log) - 1.0)
    print("no_speech_prob", got, "relative error", err, "bound", rel)
    assert (got > 0).all() and (got < 1).all() and (err <= rel).all(), (err, rel)
    # the oracle's step-0 logits: softmax at <|nospeech|>, at the tolerance a device log-prob is held to against it
    enc = om.encode(mel)
    rows = om.lm_head(om.decode_tokens(np.full((B, 1), om.start, dtype=np.int64), 0, {}, om.cross_kv(enc))[:, -1])
    ora_log = rows[:, nsp_id].astype(np.float64) - logsumexp64(rows)
    np.testing.assert_allclose(np.log(got), ora_log, atol=LOGPROB_ATOL, rtol=LOGPROB_RTOL)
    # generate-style: the same values; the ids bit-identical with the probe on and off
    rows_p, lens_p = pack_prompts([[]] * B, dims.decoder_start_token_id, dims.pad_token_id)
    m._install_rules(None)
    from whisper_context_biasing_amd import request as RQ
    m._install_rules(RQ.rules_key(dims, True, c["suppress"], c["begin"], 1.0))
    outs = []
    for probe in (True, False, True):
        w, keep = _WindowBatch(x, 3000, [0, 1, 2], [0, 0, 0], [3000] * 3).abi()
        cfg = _lib.WcbGenCfg(12, 0, 1, 0.0, 1, 0)
        ids = torch.empty(B, 12, dtype=torch.int32, device="cuda")
        lp = torch.zeros(B, 12, dtype=torch.float32, device="cuda")
        ns = torch.full((B,), -1.0, dtype=torch.float32, device="cuda")
        steps = C.c_int32(0)
        rc = lib.wcb_generate_windows(m._h, C.byref(w), B, C.byref(cfg), None, None, rows_p.ctypes.data, 1, lens_p.ctypes.data,
                                      ids.data_ptr(), lp.data_ptr(), ns.data_ptr() if probe else None, C.byref(steps), None)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((ids.cpu().numpy()[:, :steps.value], lp.cpu().numpy(), ns.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0], outs[2][0]) and np.array_equal(outs[0][2], outs[2][2])
    assert np.array_equal(outs[0][0][:, 0], ids0.cpu().numpy())
    assert np.array_equal(outs[0][2].astype(np.float64), got) and (outs[1][2] == -1.0).all()
    # the probe without the log-probs it reuses: refused
    rc = lib.wcb_generate_windows(m._h, C.byref(w), B, C.byref(cfg), None, None, rows_p.ctypes.data, 1, lens_p.ctypes.data,
                                  ids.data_ptr(), None, ns.data_ptr(), C.byref(steps), None)
    assert rc == -4
    del keep


# ------------------------------------------------------------------------------------------- 4. end to end
def e2e_kwargs(c, **kw):
    return dict(max_new_tokens=LN.MAX_NEW, suppress_tokens=c["suppress"], begin_suppress_tokens=c["begin"],
                max_initial_timestamp=LN.MAX_INIT_INDEX * 0.02, **kw)


def e2e_inputs(c):
    feats = torch.from_numpy(c["feats"])
    mask = torch.zeros(feats.shape[0], feats.shape[2], dtype=torch.int64)
    for b, n in enumerate(c["max_frames"]):
        mask[b, :int(n)] = 1
    return feats, mask


def check_against_fixture(out, b, key, row=None):
    row = b if row is None else row
    seq = out.sequences[row].cpu().numpy()
    want = E2E[key + "sequence"]
    assert np.array_equal(seq[:len(want)], want) and (seq[len(want):] == LN.e2e_case()["dims"].pad_token_id).all(), (b, seq, want)
    assert out.seeks[row] == E2E[key + "seeks"].tolist(), (b, out.seeks[row])
    segs = out.segments[row]
    assert [len(s[2]) for s in segs] == E2E[key + "seg_lens"].tolist()
    assert np.array_equal(np.asarray([s[0] for s in segs]), E2E[key + "seg_start"])
    assert np.array_equal(np.asarray([s[1] for s in segs]), E2E[key + "seg_end"])


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("cond", [False, True])
def test_end_to_end_equals_reference(cond, use_graph):
    c = LN.e2e_case()
    m = micro()
    feats, mask = e2e_inputs(c)
    kw = e2e_kwargs(c, condition_on_prev_tokens=cond, use_graph=use_graph)
    out = m.transcribe_long(feats, mask, **kw)
    ref = LN.e2e_reference(cond)
    nclip = len(LN.CLIP_SECONDS)
    for b in range(nclip):
        check_against_fixture(out, b, f"diverse_cond{int(cond)}_clip{b}_")
        st, windows = ref[b]
        assert out.window_ids[b] == [[t for t in w["ids"] if t != c["dims"].eos_token_id] for w in windows]
        np.testing.assert_allclose(out.avg_logprobs[b], [w["avg_logprob"] for w in windows], atol=LOGPROB_ATOL, rtol=LOGPROB_RTOL)
        np.testing.assert_allclose(np.log(out.no_speech_probs[b]), np.log([w["no_speech_prob"] for w in windows]),
                                   atol=LOGPROB_ATOL, rtol=LOGPROB_RTOL)
    # the batch really shrinks: the 9 s clip leaves after the first window, the 40 s clip after the second
    assert [len(s) for s in out.seeks] == [3, 2, 1]
    if cond:   # the second window's prompts really differ in length (and the first window's are the start token alone)
        p0, p1 = ref[0][1][1]["prompt"], ref[1][1][1]["prompt"]
        assert len(p0) > 1 and len(p1) > 1 and len(p0) != len(p1), (len(p0), len(p1))
        assert ref[0][1][0]["prompt"] == [] and len(ref[0][1][2]["prompt"]) > len(p0)
    # every clip alone: bitwise the same result
    for b in range(nclip):
        alone = m.transcribe_long(feats[b:b + 1], mask[b:b + 1], **kw)
        n = int((alone.sequences[0] != c["dims"].pad_token_id).sum()) if alone.sequences.shape[1] else 0
        assert torch.equal(alone.sequences[0, :n], out.sequences[b, :n]) and (out.sequences[b, n:] == c["dims"].pad_token_id).all()
        assert alone.seeks[0] == out.seeks[b] and alone.segments[0] == out.segments[b]
        np.testing.assert_allclose(alone.avg_logprobs[0], out.avg_logprobs[b], rtol=1e-5)
        np.testing.assert_allclose(alone.no_speech_probs[0], out.no_speech_probs[b], rtol=1e-5)


def test_end_to_end_from_pcm_and_reordered():
    """PCM in: the whole-recording log-mel on the device, then the same loop; clips in another order."""
    c = LN.e2e_case()
    m = micro()
    order = [2, 0, 1]
    out = m.transcribe_long(pcm=[c["pcms"][b] for b in order], **e2e_kwargs(c))
    for row, b in enumerate(order):
        check_against_fixture(out, b, f"diverse_cond0_clip{b}_", row=row)


@pytest.mark.parametrize("cond", [False, True])
def test_per_clip_bias_lists(cond):
    c = LN.e2e_case()
    m = micro()
    feats, mask = e2e_inputs(c)
    lists = LN.e2e_bias_lists()
    ref = LN.e2e_reference(cond, bias_lists=lists, lam=2.0)
    plain = LN.e2e_reference(cond)
    out = m.transcribe_long(feats, mask, bias_lists=lists, bias_boost=2.0, **e2e_kwargs(c, condition_on_prev_tokens=cond))
    for b in range(len(LN.CLIP_SECONDS)):
        st, windows = ref[b]
        for w in windows:   # the comparison is well posed: the boosted oracle resolves every step
            assert w["top2"].min() >= LN.MARGIN and w["rule5"].min() >= LN.MARGIN
        want = st.sequences()[0]
        assert np.array_equal(out.sequences[b].cpu().numpy()[:len(want)], want), b
        assert out.seeks[b] == st.seeks[0] and out.segments[b] == st.segments[0]
        assert not np.array_equal(want, plain[b][0].sequences()[0])   # the boost moved tokens


def test_skip_rule():
    c = LN.e2e_case()
    m = micro()
    feats, mask = e2e_inputs(c)
    b = 1
    w0 = LN.e2e_reference(False)[b][1][0]
    thr = dict(no_speech_threshold=0.5 * w0["no_speech_prob"], logprob_threshold=w0["avg_logprob"] + 0.5)
    st, _ = LN.transcribe_clip(c["om"], c["dims"], c["feats"][b], int(c["max_frames"][b]), c["rules"], **thr)
    assert st.skipped[0][0] and st.seeks[0][:2] == [0, 3000]
    out = m.transcribe_long(feats[b:b + 1], mask[b:b + 1], **e2e_kwargs(c, **thr))
    assert out.seeks[0] == st.seeks[0] and out.seeks[0][1] == 3000        # seek advanced by seek_num_frames
    assert out.segments[0] == st.segments[0]
    assert all(s[0] >= 30.0 for s in out.segments[0])                       # the first window yields no segment
    assert len(out.window_ids[0][0]) > 0                                    # (it was decoded, then dropped)
    off = m.transcribe_long(feats[b:b + 1], mask[b:b + 1], **e2e_kwargs(c, no_speech_threshold=None,
                                                                      logprob_threshold=thr["logprob_threshold"]))
    check_against_fixture(off, b, f"diverse_cond0_clip{b}_", row=0)


def test_bf16_margin_gated():
    """micro / `margin`, bf16: per clip, window after window, every id up to the first step whose oracle margin (top-2
    among the allowed tokens, or rule 5's) is below the 16-bit gate must equal the oracle's."""
    c = LN.e2e_case("margin")
    m = micro("bf16", "margin")
    feats, mask = e2e_inputs(c)
    out = m.transcribe_long(feats, mask, **e2e_kwargs(c))
    ref = LN.e2e_reference(False, "margin")
    checked = total = 0
    for b in range(len(LN.CLIP_SECONDS)):
        st, windows = ref[b]
        go = True
        for k, w in enumerate(windows):
            total += len(w["ids"])
            if not go or k >= len(out.window_ids[b]) or out.seeks[b][k] != st.seeks[0][k]:
                break
            got = out.window_ids[b][k]
            for t, tok in enumerate(w["ids"]):
                if min(w["top2"][t], w["rule5"][t]) < TAU:
                    go = False
                    break
                if tok != c["dims"].eos_token_id:
                    assert t < len(got) and got[t] == tok, (b, k, t, got, w["ids"])
                checked += 1
    print(f"gate long-form micro-bf16-margin: {checked}/{total} tokens checked (tau {TAU})")
    assert checked >= len(LN.CLIP_SECONDS)   # at least the first token of every clip


def test_refusals():
    c = LN.e2e_case()
    m = micro()
    feats, mask = e2e_inputs(c)
    n0 = m.debug_counter("graph_captures")
    for kw in (dict(temperature=(0.0, 0.2)), dict(temperature=0.3), dict(num_beams=2),
               dict(return_token_timestamps=True, condition_on_prev_tokens=True), dict(prompt_condition_type="x"),
               dict(prompt_ids=[5], prompt_condition_type="all-segments"), dict(suppress_tokens=[c["dims"].vocab]),
               dict(bias_lists=[[]], bias_boost=1.0)):
        with pytest.raises(ValueError):
            m.transcribe_long(feats, mask, max_new_tokens=8, **kw)
    with pytest.raises(ValueError):
        m.transcribe_long(feats, mask[:, :100], max_new_tokens=8)
    with pytest.raises(ValueError):
        m.transcribe_long(max_new_tokens=8)
    assert m.debug_counter("graph_captures") == n0   # refused before any device work
    # generate() keeps its own refusal of long features
    with pytest.raises(ValueError):
        m.generate(feats, max_length=4)
