"""CPU: the host side of the token timestamps — wcb_dtw_host (csrc/dtw.h, the recurrence the DTW kernel compiles)
against transformers' _dynamic_time_warping and the pure-f32 restatement, path for path; the numpy restatement of
the cost matrix against HF's own lines in torch f64; the word helper; argument errors. No GPU."""
import ctypes as C

import numpy as np
import pytest

import align_np as A
from whisper_context_biasing_amd import _lib
from whisper_context_biasing_amd.config import words_from_token_times


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.mark.parametrize("kind", ["grid", "normal"])
@pytest.mark.parametrize("m,S", A.DTW_SHAPES)
def test_dtw_host_equals_transformers_and_restatement(lib, m, S, kind):
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    M = A.dtw_matrices(m, S, 1000 * m + S)[kind]
    frames, text, time = A.dtw_host(lib, M, n_out=m + 3)
    rt, rj = A.dtw_f32(M)
    ht, hj = gw._dynamic_time_warping(M.astype(np.float64))   # as HF calls it: the f32 values as f64
    assert np.array_equal(rt, ht) and np.array_equal(rj, hj), "the f32 restatement left transformers' path"
    assert np.array_equal(text, ht) and np.array_equal(time, hj)
    assert np.array_equal(frames, A.frames_from_path(ht, hj, m, m + 3))
    # a path: starts at (0, 0), ends at (m - 1, S - 1), steps of (0|1, 0|1)
    assert (text[0], time[0]) == (0, 0) and (text[-1], time[-1]) == (m - 1, S - 1)
    assert set(zip(np.diff(text), np.diff(time))) <= {(1, 1), (1, 0), (0, 1)}


def test_dtw_host_without_path_and_with_row_stride(lib):
    M = A.dtw_matrices(24, 300, 5)["normal"]
    wide = np.zeros((24, 333), dtype=np.float32)
    wide[:, :300] = M
    f0, _, _ = A.dtw_host(lib, M, n_out=30)
    f1 = np.zeros(30, dtype=np.int32)
    assert lib.wcb_dtw_host(wide.ctypes.data, 24, 300, 333, f1.ctypes.data, 30, None, None, None) == 0
    assert np.array_equal(f0, f1)
    assert (f1[24:] == f1[23]).all() and (np.diff(f1) >= 0).all()
    # no rows: zeros
    f2 = np.full(4, 7, dtype=np.int32)
    assert lib.wcb_dtw_host(wide.ctypes.data, 0, 300, 333, f2.ctypes.data, 4, None, None, None) == 0
    assert (f2 == 0).all()


def test_dtw_host_argument_errors(lib):
    M = np.zeros((2, 9), dtype=np.float32)
    f = np.zeros(3, dtype=np.int32)
    p = np.zeros(16, dtype=np.int32)
    assert lib.wcb_dtw_host(None, 2, 9, 9, f.ctypes.data, 3, None, None, None) == -1
    assert lib.wcb_dtw_host(M.ctypes.data, 2, 9, 8, f.ctypes.data, 3, None, None, None) == -1      # ld < S
    assert lib.wcb_dtw_host(M.ctypes.data, 2, 0, 9, f.ctypes.data, 3, None, None, None) == -1
    assert lib.wcb_dtw_host(M.ctypes.data, 2, 9, 9, f.ctypes.data, 0, None, None, None) == -1
    assert lib.wcb_dtw_host(M.ctypes.data, 2, 9, 9, f.ctypes.data, 3, p.ctypes.data, None, None) == -1   # half a path
    assert b"path" in lib.wcb_last_error(None)


def test_matrix_restatement_equals_hf_lines_in_f64():
    """align_matrix_np against the lines of HF's _extract_token_timestamps (std(unbiased=False), mean, _median_filter,
    mean over heads) run in torch f64: weights [3][2][24][1500], whole and cropped to 97 frames."""
    torch = pytest.importorskip("torch")
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    rng = np.random.default_rng(3)
    s = rng.standard_normal((3, 2, 24, 1500)) * 2.0
    w = A.softmax64(s)
    for S_b in (1500, 97):
        for b in range(3):
            matrix = torch.from_numpy(w[b][..., :S_b])
            std = torch.std(matrix, dim=-2, keepdim=True, unbiased=False)
            mean = torch.mean(matrix, dim=-2, keepdim=True)
            matrix = gw._median_filter((matrix - mean) / std, 7).mean(dim=0)
            ours = A.align_matrix_np(w[b], 24, S_b, 7)
            np.testing.assert_allclose(ours, -matrix.numpy(), rtol=0, atol=1e-12)
    # the documented deviation: a constant column is 0 here (NaN in HF)
    w2 = w[0].copy()
    w2[:, :, 40] = 0.25
    z = A.align_matrix_np(w2, 24, 97, 1)
    assert np.isfinite(z).all() and (z[:, 40] == 0).all()


def test_words_from_token_times():
    eos = 100
    ws = np.zeros(200, dtype=np.uint8)
    ws[[5, 7, 9]] = 1
    ids = [3, 4, 5, 6, 150, 7, 9, 8, eos, eos]
    times = [0.0, 0.1, 0.5, 0.6, 0.7, 1.0, 1.5, 1.6, 1.6, 1.6]
    words = words_from_token_times(ids, times, ws, eos, audio_end=12.5)
    assert words == [(0.0, 0.5, [3, 4]), (0.5, 1.0, [5, 6]), (1.0, 1.5, [7]), (1.5, 12.5, [9, 8])]
    assert words_from_token_times([eos, eos], [0.0, 0.0], ws, eos) == []
    assert words_from_token_times([150, 6], [0.2, 0.4], ws, eos) == [(0.4, 30.0, [6])]   # the first text token starts one


def test_align_cfg_struct_matches_the_header():
    cfg, keep = _lib.align_cfg([(1, 0), (3, 2)], 5, [3000, 1800])
    assert cfg.n_heads == 2 and cfg.median_width == 5
    assert [cfg.heads[i] for i in range(4)] == [1, 0, 3, 2] and [cfg.num_frames[i] for i in range(2)] == [3000, 1800]
    cfg, keep = _lib.align_cfg()
    assert cfg.n_heads == 0 and not cfg.heads and not cfg.num_frames and cfg.median_width == 7
    assert C.sizeof(_lib.WcbAlignCfg) == 8 + 4 + 4 + 8


def test_op_argument_errors_need_no_device(lib):
    """what the op entry points refuse before they touch the device"""
    assert lib.wcb_op_dtw(None, 1, 4, 9, None, None, 5, None, None, None, None, None) == -1
    one = C.c_void_p(8)   # never dereferenced: the checks come first
    assert lib.wcb_op_dtw(one, 1, 448, 9, one, None, 448, one, None, None, None, None) == -1      # m_max > 447
    assert lib.wcb_op_dtw(one, 1, 4, 9, one, None, 3, one, None, None, None, None) == -1          # n_out < m_max
    assert lib.wcb_op_align_matrix(one, 1, 2, 4, 9, one, None, 4, one, None) == -1                # even width
    assert lib.wcb_op_align_matrix(one, 1, 2, 4, 9, one, None, 0, one, None) == -1
    assert lib.wcb_op_align_matrix(one, 1, 2, 4, 9, one, None, 17, one, None) == -4               # unsupported
    assert lib.wcb_op_align_matrix(one, 1, 0, 4, 9, one, None, 7, one, None) == -1
