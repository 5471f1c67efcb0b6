"""GPU: token-level timestamps (wcb_align).

1. wcb_op_dtw: frames and paths EQUAL to wcb_dtw_host (the same csrc/dtw.h recurrence, itself equal to transformers'
   _dynamic_time_warping: tests/test_align_host.py) — items of different (m, S) in one call; one row, the 64 / 65
   wave boundary, 130 rows, m > S, the 447-row maximum (trace in the workspace), all 1500 columns.
2. wcb_op_align_matrix against the f64 restatement (tests/align_np.py). Tolerance: 8 x the gap between HF's own lines
   run in torch f32 and in f64 on the case's inputs (measured over the 12 cases: HF's f32 gap 2.0e-7 .. 6.1e-5 at
   max |z| 1.1 .. 8, so the bound is 1.6e-6 .. 4.9e-4; the kernel, whose column statistics are f64, is 9.0e-8 ..
   4.8e-7 from the f64 result).
3. End to end, micro f32 against the oracle: (a) the frames equal wcb_dtw_host on the device's own matrix, exactly;
   (b) the matrix against the oracle's, bound = 4 x the largest change of the oracle's matrix when its cross-attention
   scores move by 5e-4 (the atol of the f32 logit parity tests): bound 0.050 .. 0.135 by clip and head list, measured
   gap 9.5e-6 .. 4.1e-5, and all 33 tokens of every case on the oracle's frame (printed); (c) shape of
   the result; (d) batch invariance; (e) model.align
   on generate's sequences equals generate(return_token_timestamps=True), also after beam and timestamp decodes.
4. bf16 (micro over the encoder output and over the K cache, tiny.en): (a), (c), (d); the two encoder layouts equal.
5. The encoder-space capture: wcb_op_align_capture against the f64 softmax of its operands (errors at most 2 % of the
   derived bound), and tiny.en bf16 head by head: each encoder-space head is nearest to the same head over the K cache.
6. Chunked passes and clip groups; two post-passes in flight; off means off (same ids, no graph captured again).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_np as A  # noqa: E402
from oracle import whisper_np as W  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.config import FRAME_SECONDS, get_dims, timestamp_ids  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_word_start  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the DTW kernel
_ITEMS = [(m, S, kind) for (m, S) in A.DTW_SHAPES for kind in ("grid", "normal")]


@pytest.mark.parametrize("group,max_m", [("workspace trace, 7 waves", 447), ("LDS trace, 3 waves", 130),
                                         ("one wave", 64)])
def test_op_dtw_equals_host(group, max_m):
    lib = _lib.load()
    items = [it for it in _ITEMS if it[0] <= max_m]
    N, m_max, S_ld = len(items), max(it[0] for it in items), max(it[1] for it in items)
    assert m_max == max_m
    M = np.full((N, m_max, S_ld), np.nan, dtype=np.float32)   # whatever lies outside an item must not matter
    for k, (m, S, kind) in enumerate(items):
        M[k, :m, :S] = A.dtw_matrices(m, S, 1000 * m + S)[kind]
    lens = np.asarray([it[0] for it in items], dtype=np.int32)
    frs = np.asarray([it[1] for it in items], dtype=np.int32)
    n_out = m_max + 2
    out = torch.full((N, n_out), -7, dtype=torch.int32, device="cuda")
    pt = torch.full((N, m_max + S_ld), -7, dtype=torch.int32, device="cuda")
    pj = torch.full((N, m_max + S_ld), -7, dtype=torch.int32, device="cuda")
    pl = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    Md, ld, fd = dev(M), dev(lens), dev(frs)
    rc = lib.wcb_op_dtw(Md.data_ptr(), N, m_max, S_ld, ld.data_ptr(), fd.data_ptr(), n_out, out.data_ptr(), pt.data_ptr(),
                        pj.data_ptr(), pl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.wcb_last_error(None)
    out, pt, pj, pl = out.cpu().numpy(), pt.cpu().numpy(), pj.cpu().numpy(), pl.cpu().numpy()
    for k, (m, S, kind) in enumerate(items):
        frames, text, time = A.dtw_host(lib, M[k, :m, :S], n_out=n_out)
        assert pl[k] == len(text), (m, S, kind, pl[k], len(text))
        assert np.array_equal(pt[k, :pl[k]], text) and np.array_equal(pj[k, :pl[k]], time), (m, S, kind)
        assert np.array_equal(out[k], frames), (m, S, kind)
    # frames alone (no path), S = the row stride (frames = NULL), zero rows for one item
    lens0 = lens.copy()
    lens0[0] = 0
    full = np.where(np.isnan(M), np.float32(0.5), M)
    out2 = torch.full((N, n_out), -7, dtype=torch.int32, device="cuda")
    full_d, lens0_d = dev(full), dev(lens0)   # (kept alive over the call)
    rc = lib.wcb_op_dtw(full_d.data_ptr(), N, m_max, S_ld, lens0_d.data_ptr(), None, n_out, out2.data_ptr(), None,
                        None, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    out2 = out2.cpu().numpy()
    assert (out2[0] == 0).all()
    for k in range(1, N):
        frames, _, _ = A.dtw_host(lib, full[k, :lens0[k]], n_out=n_out)
        assert np.array_equal(out2[k], frames), items[k]


# ------------------------------------------------------------------------------------------------ 2. the matrix kernel
@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("width", [7, 1, 3])
@pytest.mark.parametrize("heads", [1, 3])
def test_op_align_matrix_against_f64(heads, width, rot):
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    lib = _lib.load()
    ms, Ss = [2, 24, 65], [7, 97, 1500]
    items = [(ms[k], Ss[(k + rot) % 3]) for k in range(3)]
    N, m_max, S_ld = 3, 65, 1500
    rng = np.random.default_rng(100 * heads + 10 * width + rot)
    w = A.softmax64(rng.standard_normal((N, heads, m_max, S_ld)) * 2.0).astype(np.float32)
    planted = [3, 40, 777]
    for k, (m, S) in enumerate(items):
        w[k, :, :, min(planted[k], S - 1)] = np.float32(1.0 / 1024)   # std = 0: normalises to 0
    lens = np.asarray([it[0] for it in items], dtype=np.int32)
    frs = np.asarray([it[1] for it in items], dtype=np.int32)
    out = torch.full((N, m_max, S_ld), 9.0, dtype=torch.float32, device="cuda")
    w_d, lens_d, frs_d = dev(w), dev(lens), dev(frs)   # (kept alive over the call)
    rc = lib.wcb_op_align_matrix(w_d.data_ptr(), N, heads, m_max, S_ld, lens_d.data_ptr(), frs_d.data_ptr(), width,
                                 out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.wcb_last_error(None)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    gap_hf, gap, zmax = 0.0, 0.0, 0.0
    for k, (m, S) in enumerate(items):
        ref = A.align_matrix_np(w[k], m, S, width)
        # HF's lines in torch f32 and f64 on the same weights (NaN where a window meets the constant column)
        res = {}
        for dt in (torch.float32, torch.float64):
            x = torch.from_numpy(w[k][:, :m, :S]).to(dt)
            std = torch.std(x, dim=-2, keepdim=True, unbiased=False)
            z = gw._median_filter((x - torch.mean(x, dim=-2, keepdim=True)) / std, width).mean(dim=0)
            res[dt] = -z.numpy().astype(np.float64)
        # HF's result means nothing where a window holds the constant column's NaN (a sort puts it last)
        ind = np.zeros(S)
        ind[min(planted[k], S - 1)] = 1
        pad = width // 2
        touch = np.lib.stride_tricks.sliding_window_view(np.pad(ind, pad, mode="reflect") if pad else ind, width).max(axis=-1) > 0
        ok = np.isfinite(res[torch.float32]) & np.isfinite(res[torch.float64]) & ~touch[None, :]
        if ok.any():
            gap_hf = max(gap_hf, np.abs(res[torch.float32] - res[torch.float64])[ok].max())
            np.testing.assert_allclose(ref[ok], res[torch.float64][ok], rtol=0, atol=1e-12)
        gap = max(gap, np.abs(out[k, :m, :S] - ref).max())
        zmax = max(zmax, np.abs(ref).max())
        assert (out[k, m:] == 9.0).all() and (out[k, :, S:] == 9.0).all(), "wrote outside the item"
        if width == 1:
            assert (out[k, :m, min(planted[k], S - 1)] == 0).all()
    print(f"align_matrix heads={heads} width={width} items={items}: HF f32-f64 gap {gap_hf:.3g}, kernel gap {gap:.3g}, "
          f"max |z| {zmax:.3g}")
    assert gap_hf > 0
    assert gap <= 8 * gap_hf, (gap, gap_hf)


# ------------------------------------------------------------------------------------------------ 3. end to end
_CASES, _MODELS = {}, {}
NEW = 24
ATOL_F32 = 5e-4   # the atol of the f32 logit parity tests (test_forward_logits_match_reference_golden)


def case(size, B, seed=0, recipe="diverse"):
    key = (size, B, seed, recipe)
    if key not in _CASES:
        dims = get_dims(size)
        sd = make_weights(dims, seed=seed, recipe=recipe)
        pcm = synth_batch(B)
        mel = W.log_mel(pcm, dims.n_mel)
        _CASES[key] = dict(dims=dims, sd=sd, mel=mel, x=torch.from_numpy(mel).cuda())
    return _CASES[key]


def oracle_of(c):
    if "om" not in c:
        c["om"] = W.OracleModel.from_dims(c["dims"], c["sd"])
        c["enc"] = c["om"].encode(c["mel"])
    return c["om"], c["enc"]


def model(size, dtype, seed=0, recipe="diverse", **options):
    key = (size, dtype, seed, recipe, tuple(sorted(options.items())))
    if key not in _MODELS:
        dims = get_dims(size)
        _MODELS[key] = WhisperCB.from_state_dict(dims, make_weights(dims, seed=seed, recipe=recipe), dtype=dtype,
                                                 options=options)
    return _MODELS[key]


def planted(seq, P, eos):
    """generate's sequences with an EOS planted in clip 1 (then pads) and at the very start of the last clip"""
    seq = seq.clone()
    if seq.shape[0] > 1:
        seq[1, P + 9:] = eos
    if seq.shape[0] > 2:
        seq[-1, P + 1:] = eos
    return seq


def check_a_c(lib, m, seq, P, ts, mat, nf, eos):
    """(a) frames = wcb_dtw_host on the device's own matrix; (c) the shape of the result. Returns the frames."""
    B, n = seq.shape[0], seq.shape[1] - P
    ts, mat, ids = ts.cpu().numpy(), mat.cpu().numpy(), seq[:, P:].cpu().numpy()
    frames = np.rint(ts[:, P:] / FRAME_SECONDS).astype(np.int64)
    assert np.array_equal(frames.astype(np.float32) * np.float32(FRAME_SECONDS), ts[:, P:])
    assert (ts[:, :P] == 0).all()
    for b in range(B):
        rows = A.rows_of(ids[b], eos)
        S_b = (nf[b] if nf is not None else 3000) // 2
        if rows == 0:
            want = np.zeros(n, dtype=np.int64)
        else:
            want, _, _ = A.dtw_host(lib, mat[b, :rows, :S_b], n_out=n)
        assert np.array_equal(frames[b], want), (b, rows, S_b, frames[b], want)
        assert (np.diff(frames[b]) >= 0).all() and frames[b].min() >= 0 and frames[b].max() < S_b
        assert (frames[b, max(rows, 1) - 1:] == frames[b, max(rows, 1) - 1]).all()
        if rows <= 1:
            assert (frames[b] == 0).all()
    return frames


@pytest.mark.parametrize("nf", [None, [3000, 1800, 900]])
@pytest.mark.parametrize("heads", [[(0, 0), (1, 0)], None])
def test_end_to_end_micro_f32(heads, nf):
    """(f32 decodes over the cross-K cache: the handle has no encoder-space kernel for it, option "xmode" or not —
    the encoder-space capture is pinned by test_op_align_capture and test_encoder_space_heads_are_the_k_cache_heads)"""
    lib = _lib.load()
    c = case("micro", 3)
    dims = c["dims"]
    om, enc = oracle_of(c)
    m = model("micro", "f32")
    P, eos = 1, dims.eos_token_id
    kw = dict(alignment_heads=heads, num_frames=nf)
    for use_graph in (True, False):
        out = m.generate(c["x"], max_length=NEW, min_new_tokens=NEW, use_graph=use_graph, return_token_timestamps=True, **kw)
        assert out.sequences.shape == (3, P + NEW) and out.token_timestamps.shape == (3, P + NEW)
        ref_ids = om.generate(c["mel"], enc=enc, max_length=NEW, min_new_tokens=NEW, trim=False)
        assert np.array_equal(out.sequences[:, P:].cpu().numpy(), ref_ids)
        # (e) the stand-alone call on those sequences
        enc_d = m.encode(c["x"])
        ts, mat = m.align(enc_d, out.sequences, P, return_matrix=True, **kw)
        assert torch.equal(ts, out.token_timestamps), (use_graph, ts, out.token_timestamps)
        check_a_c(lib, m, out.sequences, P, ts, mat, nf, eos)
    # clips of different lengths: an EOS planted in two of them
    seq = planted(out.sequences, P, eos)
    ts, mat = m.align(enc_d, seq, P, return_matrix=True, **kw)
    frames = check_a_c(lib, m, seq, P, ts, mat, nf, eos)
    # (d) every clip alone
    for b in range(3):
        one = m.align(enc_d[b:b + 1], seq[b:b + 1], P, num_frames=None if nf is None else nf[b:b + 1], alignment_heads=heads)
        assert torch.equal(one[0], ts[b]), (b, one, ts[b])
    # (b) the matrix against the oracle's, the bound from the oracle alone
    hl = heads if heads is not None else A.default_heads(dims)
    gens = seq[:, P:].cpu().numpy()
    S_b = [(nf[b] if nf is not None else 3000) // 2 for b in range(3)]
    tf = np.concatenate([seq[:, :P].cpu().numpy(), gens[:, :-1]], axis=1)
    scores = A.oracle_cross_scores(om, enc, tf)
    ref = A.oracle_matrices(scores, hl, P, gens, eos, S_b)
    rng = np.random.default_rng(11)
    moved = A.oracle_matrices(scores, hl, P, gens, eos, S_b,
                              perturb=lambda l, h, b, shape: ATOL_F32 * rng.choice([-1.0, 1.0], size=shape))
    mat = mat.cpu().numpy()
    agree = near = total = 0
    for b in range(3):
        rows = ref[b].shape[0]
        if rows == 0:
            continue
        bound = 4 * np.abs(moved[b] - ref[b]).max()
        gap = np.abs(mat[b, :rows, :S_b[b]] - ref[b]).max()
        print(f"micro f32 heads={heads} nf={nf} clip {b}: rows {rows}, matrix gap {gap:.3g}, bound {bound:.3g}")
        assert gap <= bound, (b, gap, bound)
        text, time = A.dtw_f32(ref[b].astype(np.float32))
        want = A.frames_from_path(text, time, rows, NEW)
        agree += int((want[:rows] == frames[b, :rows]).sum())
        near += int((np.abs(want[:rows] - frames[b, :rows]) <= 1).sum())
        total += rows
    print(f"micro f32 heads={heads} nf={nf}: {agree} / {total} tokens on the oracle's frame, {near} within 1")


def test_align_equals_generate_for_beam_and_timestamp_decodes():
    c = case("micro", 3)
    dims = c["dims"]
    m = model("micro", "f32")
    enc_d = m.encode(c["x"])
    ts0, nots = timestamp_ids(dims)
    sot = dims.decoder_start_token_id
    for kw, P in ((dict(num_beams=2), 1), (dict(return_timestamps=True, prompt_ids=[sot + 1, sot + 2]), 3),
                  (dict(output_logprobs=True, temperature=0.7, seed=5), 1)):
        out = m.generate(c["x"], max_length=12, min_new_tokens=6, return_token_timestamps=True, **kw)
        plain = m.generate(c["x"], max_length=12, min_new_tokens=6, return_dict_in_generate=True, **kw)
        assert torch.equal(out.sequences, plain.sequences), kw
        ts = m.align(enc_d, out.sequences, P)
        assert torch.equal(ts, out.token_timestamps), (kw, ts, out.token_timestamps)
        assert (out.token_timestamps[:, :P] == 0).all()
        if "return_timestamps" in kw:
            assert out.segments is not None
    # temperature fallback: the explicit-encoder form over the final sequences
    out = m.generate(c["x"], max_length=12, min_new_tokens=6, temperature=(0.0, 0.5), logprob_threshold=-0.01,
                     return_token_timestamps=True)
    assert torch.equal(m.align(enc_d, out.sequences, 1), out.token_timestamps)


def test_words_and_argument_errors():
    c = case("micro", 3)
    dims = c["dims"]
    m = model("micro", "f32")
    m.set_word_start(synth_word_start(dims.eos_token_id, dims.vocab))
    try:
        out = m.generate(c["x"], max_length=12, min_new_tokens=12, return_token_timestamps=True, num_frames=[3000, 2000, 1000])
    finally:
        m.set_word_start(None)
    assert len(out.words) == 3
    ids, ts = out.sequences[:, 1:].cpu().numpy(), out.token_timestamps[:, 1:].cpu().numpy()
    for b, words in enumerate(out.words):
        assert [t for w in words for t in w[2]] == [int(t) for t in ids[b] if t < dims.eos_token_id]
        assert words[-1][1] == [30.0, 20.0, 10.0][b] and words[0][0] == float(ts[b][ids[b] < dims.eos_token_id][0])
        assert all(a[1] == b_[0] for a, b_ in zip(words, words[1:]))
    n0 = m.debug_counter("graph_captures")
    for bad in (dict(median_filter_width=4), dict(median_filter_width=0), dict(median_filter_width=17),
                dict(alignment_heads=[(2, 0)]), dict(alignment_heads=[(0, 1)]), dict(alignment_heads=[]),
                dict(num_frames=[3000, 3000]), dict(num_frames=[3000, 3000, 13]), dict(num_frames=[3000, 3000, 3002]),
                dict(block=False)):
        with pytest.raises(ValueError):
            m.generate(c["x"], max_length=4, return_token_timestamps=True, **bad)
    assert m.debug_counter("graph_captures") == n0   # refused before any work
    enc_d = m.encode(c["x"])
    with pytest.raises(ValueError):
        m.align(enc_d, out.sequences, 0)
    with pytest.raises(ValueError):
        m.align(enc_d[:2], out.sequences, 1)
    # the library's own checks
    lib = _lib.load()
    ids_d = out.sequences[:, 1:].to(torch.int32).contiguous()
    fr = torch.zeros(3, 12, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(enc, B, **kw):
        cfg, keep = _lib.align_cfg(**kw)
        return lib.wcb_align(m._h, enc, B, ids_d.data_ptr(), 12, 12, None, 1, C.byref(cfg), fr.data_ptr(), None, st)
    assert call(enc_d.data_ptr(), 3, heads=[(0, 5)]) == -1
    assert call(enc_d.data_ptr(), 3, median_width=2) == -1
    assert call(enc_d.data_ptr(), 3, num_frames=[3000, 3000, 12]) == -1
    assert call(enc_d.data_ptr(), 65) == -1
    assert call(None, 3) == 0       # refused calls took nothing: the generate above still holds its encoder state
    assert call(enc_d.data_ptr(), 3) == 0
    assert call(None, 3) == -2      # the explicit-encoder call took a decode context since the last generate
    m.generate(c["x"], max_length=4)
    assert call(None, 2) == -2      # another batch size
    assert call(None, 3) == 0


# ------------------------------------------------------------------------------------------------ 4. bf16
@pytest.mark.parametrize("size,B,options", [("micro", 2, dict(xmode=1)), ("micro", 2, dict(xmode=0)), ("tiny.en", 2, dict())])
def test_bf16_frames_follow_the_device_matrix(size, B, options):
    """(a), (c), (d) in bf16, where the capture reads the encoder output (xmode 1) or the cross-K cache (xmode 0).
    (d) holds bit for bit while batch and single-clip passes run the same projection kernels: B x 24 <= 64 rows here
    (the 16-bit decoder projections change kernels above 64 rows, f32 never). In encoder space the fragment-major and
    the row layout of the encoder output must give the same weights bit for bit (the same products in the same
    order): checked on the heads of layer 0."""
    lib = _lib.load()
    seed, recipe = (1, "margin") if size == "tiny.en" else (0, "diverse")
    c = case(size, B, seed, recipe)
    m = model(size, "bf16", seed, recipe, **options)
    eos, P = c["dims"].eos_token_id, 1
    out = m.generate(c["x"], max_length=NEW, min_new_tokens=NEW, return_token_timestamps=True)
    enc_d = m.encode(c["x"])
    ts, mat = m.align(enc_d, out.sequences, P, return_matrix=True)
    assert torch.equal(ts, out.token_timestamps)
    seq = planted(out.sequences, P, eos)
    nf = [3000, 1700][:B]
    ts, mat = m.align(enc_d, seq, P, return_matrix=True, num_frames=nf)
    check_a_c(lib, m, seq, P, ts, mat, nf, eos)
    for b in range(B):
        one = m.align(enc_d[b:b + 1], seq[b:b + 1], P, num_frames=nf[b:b + 1])
        assert torch.equal(one[0], ts[b]), (b, one, ts[b])
    if options.get("xmode", 1) == 1:
        # every head of layer 0: its query precedes every cross-attention, whose own kernels (not the capture) round
        # their partial sums differently by layout at d % 128 == 0 and so move the later layers' queries
        l0 = [(0, h) for h in range(c["dims"].n_heads)]
        ts_f, mat_f = m.align(enc_d, seq, P, return_matrix=True, num_frames=nf, alignment_heads=l0)
        m.set_option("xenc_fm", 0)
        try:
            ts_r, mat_r = m.align(enc_d, seq, P, return_matrix=True, num_frames=nf, alignment_heads=l0)
        finally:
            m.set_option("xenc_fm", 1)
        gens = seq[:, P:].cpu().numpy()
        for b in range(B):
            rows = A.rows_of(gens[b], eos)
            assert torch.equal(mat_r[b, :rows, :nf[b] // 2], mat_f[b, :rows, :nf[b] // 2]), "encoder layouts differ"
        assert torch.equal(ts_r, ts_f)


def test_encoder_space_heads_are_the_k_cache_heads():
    """The wiring of the encoder-space capture (q' = W_k,h^T q_h of the right layer and head against the clip's own
    encoder output) in a real decoder: tiny.en bf16 (4 layers x 6 heads, d = 384), the same sequences aligned one
    head at a time (width 1: the matrix is that head's negated z-scores) by a handle in encoder space (xmode 1) and
    by one over the cross-K cache (xmode 0), the path the f32 tests pin to the oracle. The two compute the same
    scores q.k = q'.enc up to what each rounds to bf16, so for every clip each of the 24 encoder-space heads must be
    nearest (mean |difference|) to the SAME (layer, head) among the 24 K-cache ones — no tolerance: a wrong head,
    layer, clip or key order matches another head or none. (A bound on the difference itself, derived from one bf16
    rounding of each operand on the oracle's scores, comes out at 7 .. 18 on z-scores of at most 4.8 and pins
    nothing; measured: 0.18 .. 0.20 with the default heads, 0.66 .. 1.24 with one or two heads. The capture
    kernel's own arithmetic is pinned by test_op_align_capture.)"""
    B, P = 2, 1
    c = case("tiny.en", B, 1, "margin")
    dims = c["dims"]
    m1 = model("tiny.en", "bf16", 1, "margin")
    m0 = model("tiny.en", "bf16", 1, "margin", xmode=0)
    seq = m1.generate(c["x"], max_length=NEW, min_new_tokens=NEW, return_dict_in_generate=True).sequences
    all_heads = [(l, h) for l in range(dims.n_layers) for h in range(dims.n_heads)]
    mats = []
    for m in (m1, m0):
        enc_d = m.encode(c["x"])
        mats.append(np.stack([m.align(enc_d, seq, P, alignment_heads=[lh], median_filter_width=1,
                                      return_matrix=True)[1].cpu().numpy() for lh in all_heads]))   # [24][B][23][1500]
    for b in range(B):
        d = np.abs(mats[0][:, None, b] - mats[1][None, :, b]).mean(axis=(2, 3))   # [encoder-space head][K-cache head]
        own, other = np.diag(d), (d + np.diag(np.full(len(all_heads), np.inf))).min(axis=1)
        print(f"tiny.en bf16 clip {b}: mean |z difference| to the same head {own.min():.3g} .. {own.max():.3g}, "
              f"to the nearest other head {other.min():.3g} .. {other.max():.3g}")
        assert (d.argmin(axis=1) == np.arange(len(all_heads))).all(), (b, d.argmin(axis=1))
    # the default head list, for the record
    ma, mb = (m.align(m.encode(c["x"]), seq, P, return_matrix=True)[1].cpu().numpy() for m in (m1, m0))
    print(f"tiny.en bf16 default heads: encoder space vs K cache, largest |difference| {np.abs(ma - mb).max():.3g}")


# ------------------------------------------------------------------------------------------------ the capture kernel
@pytest.mark.parametrize("dtype,layout,S", [("bf16", 1, 77), ("bf16", 2, 1500), ("f16", 2, 100), ("f16", 1, 1500),
                                            ("bf16", 0, 1500), ("f32", 0, 77)])
def test_op_align_capture(dtype, layout, S):
    """wcb_op_align_capture against the f64 softmax of the very operands (already rounded to the dtype): 3 clips of
    which the last two are kept, 6 heads of which (4, 1, 5) are selected, 21 positions per clip from position 5 with a
    3-token prefix (rows 2 .. 19 of 20 written, none else), S not a multiple of 16 or of 4 in the row layouts.
    Bound: the products are exact in f32, the f32 accumulation of dim + 1 terms is within (dim + 1) 2^-24 sum |q k| of
    the exact score (ds); a weight is exp(s - max) / sum: relative error 2 ds from the two scores, plus 128 x 2^-24 for
    expf, the <= 96 + 8 additions of a lane's and the workgroup's sum, and the division."""
    lib = _lib.load()
    tdt, code = {"bf16": (torch.bfloat16, 0), "f16": (torch.float16, 1), "f32": (torch.float32, 2)}[dtype]
    clips, H, rps, pos0, P, nrow, clip0, nclip = 3, 6, 21, 5, 3, 20, 1, 2
    dim = 64 if layout == 0 else 384
    heads = np.asarray([4, 1, 5], dtype=np.int32)
    g = torch.Generator().manual_seed(7 * S + layout)
    q = (torch.randn(clips * rps, H * dim, generator=g) * 0.25).to(tdt).cuda()
    if layout == 0:
        keys = torch.randn(clips, H, S, 64, generator=g).to(tdt).cuda()
    else:
        keys = torch.randn(clips, S, dim, generator=g).to(tdt).cuda()
    w = torch.full((nclip, len(heads), nrow, S), 9.0, dtype=torch.float32, device="cuda")
    rc = lib.wcb_op_align_capture(code, q.data_ptr(), H * dim, dim, keys.data_ptr(), layout, clips, H, dim, S, rps, pos0, P,
                                  nrow, clip0, nclip, heads.ctypes.data, len(heads), w.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.wcb_last_error(None)
    w = w.cpu().numpy().astype(np.float64)
    qh = q.float().cpu().numpy().astype(np.float64).reshape(clips, rps, H, dim)
    kh = keys.float().cpu().numpy().astype(np.float64)
    worst = 0.0
    for ci in range(nclip):
        for si, h in enumerate(heads):
            kk = kh[clip0 + ci, h] if layout == 0 else kh[clip0 + ci]          # [S, dim]
            for i in range(nrow):
                j = i + P - pos0
                if not 0 <= j < rps:
                    assert (w[ci, si, i] == 9.0).all(), (ci, si, i)
                    continue
                qv = qh[clip0 + ci, j, h]
                ref = A.softmax64(kk @ qv)
                ds = (dim + 1) * 2.0 ** -24 * (np.abs(kk) @ np.abs(qv)).max()
                rel = 2 * ds + 128 * 2.0 ** -24
                err = np.abs(w[ci, si, i] - ref)
                worst = max(worst, (err / (rel * ref + 1e-300)).max())
                assert (err <= rel * ref + 1e-300).all(), (ci, h, i, err.max(), rel)
                assert abs(w[ci, si, i].sum() - 1) < 1e-4
    print(f"align_capture {dtype} layout {layout} S={S}: worst error / bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------ passes and groups
def test_chunked_passes_and_clip_groups_f32():
    """11 clips of 24 tokens after a 3-token prompt: the teacher-forced pass takes two chunks (23 positions, not a
    multiple of the capture's 16-row tile, then 3; the prompt ends inside the first), and with the weights workspace
    bounded at 1 MiB (option "align_ws") the clips go in two groups (7 + 4). Every clip's frames follow its own matrix,
    the matrix is within the oracle's bound, and the grouped result equals the ungrouped one bit for bit."""
    c = case("micro", 11)
    dims = c["dims"]
    m = model("micro", "f32")
    sot = dims.decoder_start_token_id
    out = m.generate(c["x"], max_length=NEW, min_new_tokens=NEW, prompt_ids=[sot + 1, sot + 2], return_token_timestamps=True)
    P = 3
    seq = planted(out.sequences, P, dims.eos_token_id)
    enc_d = m.encode(c["x"])
    nf = [3000 - 100 * b for b in range(11)]
    ts, mat = m.align(enc_d, seq, P, num_frames=nf, return_matrix=True)
    assert torch.equal(m.align(enc_d, out.sequences, P), out.token_timestamps)
    gens = seq[:, P:].cpu().numpy()
    check_a_c(_lib.load(), m, seq, P, ts, mat, nf, dims.eos_token_id)
    # the matrix against the oracle's, bound as in test_end_to_end_micro_f32 (b)
    om, enc = oracle_of(c)
    tf = np.concatenate([seq[:, :P].cpu().numpy(), gens[:, :-1]], axis=1)
    scores = A.oracle_cross_scores(om, enc, tf)
    hl, S_b = A.default_heads(dims), [f // 2 for f in nf]
    ref = A.oracle_matrices(scores, hl, P, gens, dims.eos_token_id, S_b)
    rng = np.random.default_rng(14)
    moved = A.oracle_matrices(scores, hl, P, gens, dims.eos_token_id, S_b,
                              perturb=lambda l, h, b, shape: ATOL_F32 * rng.choice([-1.0, 1.0], size=shape))
    mat_h = mat.cpu().numpy()
    for b in range(11):
        rows = ref[b].shape[0]
        bound, gap = 4 * np.abs(moved[b] - ref[b]).max(), np.abs(mat_h[b, :rows, :S_b[b]] - ref[b]).max()
        assert gap <= bound, (b, gap, bound)
    m.set_option("align_ws", 1)
    try:
        ts_g, mat_g = m.align(enc_d, seq, P, num_frames=nf, return_matrix=True)
    finally:
        m.set_option("align_ws", 1024)
    assert torch.equal(ts_g, ts)
    for b in range(11):
        rows = A.rows_of(gens[b], dims.eos_token_id)
        assert torch.equal(mat_g[b, :rows, :nf[b] // 2], mat[b, :rows, :nf[b] // 2]), b


def test_two_post_passes_in_flight():
    """generate(block=False) -> align -> generate(block=False) -> align with no host wait in between: the two
    post-passes run in different decode contexts (different streams) and share the handle's workspaces, so the
    second must wait for the first. Frames equal to the blocking calls'."""
    c = case("micro", 3)
    m = model("micro", "f32")
    xs = [c["x"], c["x"].flip(0).contiguous()]
    kw = dict(max_length=NEW, min_new_tokens=NEW)
    want = [m.generate(x, return_token_timestamps=True, **kw) for x in xs]
    akw = m._align_args(3, None, None, 7)
    sot = [c["dims"].decoder_start_token_id]
    for _ in range(3):
        ids, frames = [], []
        for x in xs:
            ids.append(m.generate(x, block=False, **kw))              # int32 device view, valid after synchronize()
            frames.append(m._align_call(None, ids[-1], sot, akw, None))
        m.synchronize()
        for k in range(2):
            assert torch.equal(ids[k].to(torch.int64), want[k].sequences[:, 1:])
            got = frames[k].to(torch.float32) * FRAME_SECONDS
            assert torch.equal(got, want[k].token_timestamps[:, 1:]), (k, got, want[k].token_timestamps)


# ------------------------------------------------------------------------------------------------ 5. off means off
def test_off_means_off():
    c = case("micro", 3)
    m = model("micro", "f32")
    kw = dict(max_length=12, min_new_tokens=12)
    plain = m.generate(c["x"], **kw).cpu().numpy()
    for on in (True, False, True, False, True, False):   # both kinds in both decode contexts; the workspaces grow once
        m.generate(c["x"], return_token_timestamps=on, **kw)
    n0 = m.debug_counter("graph_captures")
    for on in (False, True, True, False, True, False, False, True):
        out = m.generate(c["x"], return_token_timestamps=on, **kw)
        ids = out.sequences[:, 1:].cpu().numpy() if on else out.cpu().numpy()
        assert np.array_equal(ids, plain), on
    assert m.debug_counter("graph_captures") == n0
