"""Helpers of the token-timestamp tests (not a test module): the numpy restatement of the semantics (include/wcb.h,
DESIGN.md §5e), the oracle decoder's layer loop returning the cross-attention scores, and the pure-f32 DTW."""
import ctypes as C

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------- DTW
def dtw_f32(matrix):
    """transformers' _dynamic_time_warping restated with every cost in f32 (an f32 matrix: the same sums, since
    the f64 sum of two f32 values rounds to their f32 sum). Returns (text_indices, time_indices)."""
    matrix = np.asarray(matrix, dtype=F32)
    m, S = matrix.shape
    inf = F32(np.inf)
    prev = np.full(S + 1, inf, dtype=F32)
    prev[0] = 0
    trace = np.zeros((m + 1, S + 1), dtype=np.int8)
    for i in range(1, m + 1):
        cur = np.full(S + 1, inf, dtype=F32)
        row = matrix[i - 1]
        tr = trace[i]
        for j in range(1, S + 1):
            c0, c1, c2 = prev[j - 1], prev[j], cur[j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cur[j] = row[j - 1] + c
            tr[j] = t
        prev = cur
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = m, S
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.asarray(text[::-1], dtype=np.int64), np.asarray(time[::-1], dtype=np.int64)


def frames_from_path(text, time, m, n_out):
    """HF's jump times as frame indices: the time index of the first path cell of every row; rows >= m repeat the
    last row's frame; m <= 1: zeros."""
    out = np.zeros(n_out, dtype=np.int64)
    if m <= 1 or len(text) == 0:
        return out
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    jt = time[jumps]
    assert len(jt) == m, (len(jt), m)
    out[:m] = jt
    out[m:] = jt[-1]
    return out


def dtw_matrices(m, S, seed):
    """The two kinds of test matrix: integers / 256 in [-4, 4] (tie-heavy, every partial sum exact in f32) and
    random normal f32."""
    rng = np.random.default_rng(seed)
    grid = (rng.integers(-1024, 1025, size=(m, S)).astype(np.float64) / 256.0).astype(F32)
    # few distinct values: ties on most cells
    coarse = (rng.integers(-2, 3, size=(m, S)).astype(np.float64) * 0.5).astype(F32)
    grid[:, : S // 2] = coarse[:, : S // 2]
    return {"grid": grid, "normal": rng.standard_normal((m, S)).astype(F32)}


DTW_SHAPES = [(1, 7), (2, 9), (63, 70), (64, 64), (65, 130), (130, 97), (447, 96), (24, 1500)]


def dtw_host(lib, M, n_out=None):
    """wcb_dtw_host on one matrix: (frames [n_out], text, time)."""
    M = np.ascontiguousarray(M, dtype=F32)
    m, S = M.shape
    n_out = n_out or m + 1
    frames = np.zeros(n_out, dtype=np.int32)
    pt = np.zeros(m + S, dtype=np.int32)
    pj = np.zeros(m + S, dtype=np.int32)
    ln = C.c_int32(0)
    rc = lib.wcb_dtw_host(M.ctypes.data, m, S, S, frames.ctypes.data, n_out, pt.ctypes.data, pj.ctypes.data,
                          C.addressof(ln))
    assert rc == 0, rc
    return frames, pt[: ln.value].astype(np.int64), pj[: ln.value].astype(np.int64)


# ---------------------------------------------------------------------------------------------- the matrix
def median_filter_np(x, width):
    """HF's _median_filter along the last axis: reflect padding, the middle of every sorted window."""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def align_matrix_np(w, m, S_b, width=7, dtype=np.float64):
    """w [heads][rows >= m][S >= S_b] of one clip -> M [m][S_b] = -(mean over heads of the median-filtered,
    column-normalised weights); a column with std 0 normalises to 0 (HF: NaN)."""
    x = np.asarray(w, dtype=dtype)[:, :m, :S_b]
    mean = x.mean(axis=-2, keepdims=True)
    std = x.std(axis=-2, keepdims=True)   # population
    z = np.where(std > 0, (x - mean) / np.where(std > 0, std, 1), 0).astype(dtype)
    return -(median_filter_np(z, width).mean(axis=0))


def rows_of(gen, eos):
    """m = min(first EOS, n - 1) of one clip's generated ids."""
    gen = np.asarray(gen)
    hit = np.flatnonzero(gen == eos)
    e = int(hit[0]) if len(hit) else len(gen)
    return min(e, len(gen) - 1)


def default_heads(dims):
    return [(l, h) for l in range(dims.n_layers // 2, dims.n_layers) for h in range(dims.n_heads)]


# ---------------------------------------------------------------------------------------------- the oracle decoder
def oracle_cross_scores(om, enc, ids):
    """OracleModel.decode_tokens' layer loop over teacher-forced `ids` [B, T] (positions 0 .. T-1, no cache),
    also returning the scaled cross-attention scores q·k of every layer: a list of [B, H, T, S] f32."""
    from oracle.whisper_np import layer_norm, linear, gelu, softmax
    ids = np.asarray(ids)
    B, T = ids.shape
    hd = om.d // om.H
    xkv = om.cross_kv(enc)
    x = (om.w("model.decoder.embed_tokens.weight")[ids] +
         om.w("model.decoder.embed_positions.weight")[:T][None]).astype(F32)
    scores = []
    for i in range(om.L):
        p = f"model.decoder.layers.{i}."
        h = layer_norm(x, om.w(p + "self_attn_layer_norm.weight"), om.w(p + "self_attn_layer_norm.bias"))
        a = p + "self_attn."
        q = (linear(h, om.w(a + "q_proj.weight"), om.w(a + "q_proj.bias")) * F32(hd ** -0.5)).astype(F32)
        k = linear(h, om.w(a + "k_proj.weight"))
        v = linear(h, om.w(a + "v_proj.weight"), om.w(a + "v_proj.bias"))
        q = q.reshape(B, T, om.H, hd).transpose(0, 2, 1, 3)
        k = k.reshape(B, T, om.H, hd).transpose(0, 2, 1, 3)
        v = v.reshape(B, T, om.H, hd).transpose(0, 2, 1, 3)
        s = np.matmul(q, k.transpose(0, 1, 3, 2)).astype(F32)
        s = np.where(np.arange(T)[None, :] <= np.arange(T)[:, None], s, F32(-np.inf))
        o = np.matmul(softmax(s), v).astype(F32).transpose(0, 2, 1, 3).reshape(B, T, om.d)
        x = (x + linear(o, om.w(a + "out_proj.weight"), om.w(a + "out_proj.bias"))).astype(F32)
        h = layer_norm(x, om.w(p + "encoder_attn_layer_norm.weight"), om.w(p + "encoder_attn_layer_norm.bias"))
        c = p + "encoder_attn."
        q = (linear(h, om.w(c + "q_proj.weight"), om.w(c + "q_proj.bias")) * F32(hd ** -0.5)).astype(F32)
        q = q.reshape(B, T, om.H, hd).transpose(0, 2, 1, 3)
        ck, cv = xkv[i]
        s = np.matmul(q, ck.transpose(0, 1, 3, 2)).astype(F32)
        scores.append(s)
        o = np.matmul(softmax(s), cv).astype(F32).transpose(0, 2, 1, 3).reshape(B, T, om.d)
        x = (x + linear(o, om.w(c + "out_proj.weight"), om.w(c + "out_proj.bias"))).astype(F32)
        h = layer_norm(x, om.w(p + "final_layer_norm.weight"), om.w(p + "final_layer_norm.bias"))
        h = gelu(linear(h, om.w(p + "fc1.weight"), om.w(p + "fc1.bias")))
        x = (x + linear(h, om.w(p + "fc2.weight"), om.w(p + "fc2.bias"))).astype(F32)
    return scores


def softmax64(s):
    s = np.asarray(s, dtype=np.float64)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def oracle_matrices(scores, heads, P, gens, eos, S_b, width=7, perturb=None):
    """Per clip the cost matrix [m][S_b] (f64) from the oracle's scores: rows = positions P + i, softmax over all
    frames, then the restatement. `perturb` (f64, broadcastable to a score array) is added to the scores."""
    out = []
    for b, gen in enumerate(gens):
        m = rows_of(gen, eos)
        w = []
        for (l, h) in heads:
            s = scores[l][b, h, P:P + m].astype(np.float64)
            if perturb is not None:
                s = s + perturb(l, h, b, s.shape)
            w.append(softmax64(s))
        out.append(align_matrix_np(np.stack(w) if m else np.zeros((len(heads), 0, scores[0].shape[-1])), m, S_b[b],
                                   width))
    return out
