"""CPU: the temperature-sampling entry points are declared in include/wcb.h with the stated arity, exported by
libwcb.so and bound in the ctypes table; the declarations they sit beside are textually unchanged; the noise the
kernels compile (csrc/sample.h through wcb_sample_noise, host side: no GPU) equals the numpy restatement kept here;
clip_seeds and compression_ratio do what generate() documents."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from whisper_context_biasing_amd import _lib
from whisper_context_biasing_amd.model import clip_seeds, compression_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wcb.h")
NEW = {"wcb_generate_sampled": 13, "wcb_decode_enable_sampling": 4, "wcb_op_lm_head_sample": 15, "wcb_sample_noise": 5}
UNCHANGED = {
    "wcb_generate": "wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias, "
                    "const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream",
    "wcb_generate_biased": "wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias_batch* bb, "
                           "const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream",
    "wcb_generate_scored": "wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias, "
                           "const wcb_bias_batch* bb, const int32_t* prefix, int prefix_len, int32_t* out_ids, "
                           "float* out_logprobs, float* out_seq_scores, int32_t* out_steps, void* stream",
    "wcb_decode_begin": "wcb_handle* h, const void* enc, int B, int num_beams, const int32_t* prefix, int prefix_len, "
                        "float bias_boost, int min_new_tokens, wcb_state** out, void* stream",
    "wcb_decode_step": "wcb_handle* h, wcb_state* st, const wcb_bias* bias, int32_t* next_ids, float* scores, void* stream",
    "wcb_decode_enable_logprobs": "wcb_handle* h, wcb_state* st",
    "wcb_op_lm_head_lse": "int dtype, const void* A, const void* W, int M, int V, int K, int walkers, float* logits, long ld, "
                          "float* lse, int32_t* argmax, void* stream",
}


def declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(wcb_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_declares_entry_point(name):
    decl = declarations()
    assert name in decl, name
    assert len(decl[name].split(",")) == NEW[name], decl[name]
    assert len(_lib.SIGNATURES[name][1]) == NEW[name]


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_existing_signatures_are_unchanged(name):
    assert re.sub(r"\s+", " ", declarations()[name]) == UNCHANGED[name]


def test_gen_cfg_layout_is_unchanged_and_sample_cfg_is_bound():
    assert [f[0] for f in _lib.WcbGenCfg._fields_] == ["max_new_tokens", "min_new_tokens", "num_beams", "bias_boost",
                                                       "use_graph", "async_out"]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} wcb_gen_cfg;", src).group(1)
    assert re.sub(r"\s+", " ", body).strip() == ("int max_new_tokens; int min_new_tokens; int num_beams; float bias_boost; "
                                                 "int use_graph; int async_out;")
    body = re.search(r"typedef struct \{([^}]*)\} wcb_sample_cfg;", src).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "float temperature; const uint64_t* seeds;"
    assert [(n, t) for n, t in _lib.WcbSampleCfg._fields_] == [("temperature", C.c_float), ("seeds", C.POINTER(C.c_uint64))]
    assert C.sizeof(_lib.WcbSampleCfg) == 16 and _lib.WcbSampleCfg.seeds.offset == 8


def test_library_exports_the_entry_points():
    _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (wcb_[a-z_0-9]+)$", out, flags=re.M))
    assert not [s for s in NEW if s not in exported]
    lib = _lib.load()
    # null handles / pointers are refused with a status before any device is touched
    assert lib.wcb_generate_sampled(None, None, 1, None, None, None, None, None, 1, None, None, None, None) == -1
    assert lib.wcb_decode_enable_sampling(None, None, 1.0, None) == -1
    assert lib.wcb_op_lm_head_sample(_lib.WCB_F32, None, None, 3, 649, 64, 0, 1.0, None, 0, None, 649, None, None, None) == -1
    assert lib.wcb_sample_noise(1, 0, 0, 4, None) == -1


# ------------------------------------------------------------------------------------ the noise, restated in numpy
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds on uint64 arrays holding 32-bit words: ctr 4 arrays, key 2 ints."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniforms(seed, step, v):
    """u(seed, step, v) as float64 (the f32 value is exact, so this is the kernels' u bit for bit)"""
    v = np.asarray(v, dtype=np.uint64)
    z = np.zeros_like(v)
    out = philox4x32_10((v >> np.uint64(2), z + np.uint64(step), z, z), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    r = np.choose((v & np.uint64(3)).astype(np.int64), out)
    return ((r >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def noise64(seed, step, v):
    return -np.log(-np.log(uniforms(seed, step, v)))


def test_restated_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(x) for x in philox4x32_10([np.uint64(c) for c in ctr], key))
        assert got == want, ([hex(g) for g in got], [hex(w) for w in want])


@pytest.mark.parametrize("seed", [0x0123456789ABCDEF, 0xFFFFFFFF00000007])
@pytest.mark.parametrize("step", [0, 5])
def test_sample_noise_matches_restatement(seed, step):
    lib = _lib.load()
    v0, n = 3, 4099   # straddles the 4-token Philox blocks at both ends
    out = np.empty(n, dtype=np.float32)
    assert lib.wcb_sample_noise(seed, step, v0, n, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    v = np.arange(v0, v0 + n)
    u = uniforms(seed, step, v)
    assert (u > 0).all() and (u < 1).all()
    assert (u.astype(np.float32).astype(np.float64) == u).all()   # exact in f32
    g64 = noise64(seed, step, v)
    # g = -logf(-logf(u)): each logf within 1 f32 spacing of its result (the accurate logf), and the inner one's
    # error e on w = -log u moves log w by e / w <= spacing(w) / w <= 2^-23 — under one spacing of g wherever
    # |g| >= 1, and under spacing(1) elsewhere. Bound: 2 spacings of max(|g|, 1), plus one for the final rounding.
    tol = 3 * np.spacing(np.maximum(np.abs(g64), 1.0).astype(np.float32)).astype(np.float64)
    err = np.abs(out.astype(np.float64) - g64)
    assert (err <= tol).all(), (err.max(), tol.min(), int(np.argmax(err / tol)))
    assert np.isfinite(out).all()
    # neighbouring tokens, steps and seeds draw different noise
    assert len(np.unique(out)) > n - 8
    other = np.empty(n, dtype=np.float32)
    assert lib.wcb_sample_noise(seed ^ 1, step, v0, n, other.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert (other != out).mean() > 0.99
    assert lib.wcb_sample_noise(seed, step + 1, v0, n, other.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert (other != out).mean() > 0.99


# ------------------------------------------------------------------------------------------------------ clip_seeds
def test_clip_seeds_are_deterministic_distinct_and_split_invariant():
    vals = {}
    for attempt in range(6):
        whole = clip_seeds(1234, 0, 130, attempt=attempt)
        assert whole.dtype == np.uint64 and whole.shape == (130,)
        assert np.array_equal(whole, clip_seeds(1234, 0, 130, attempt=attempt))
        split = np.concatenate([clip_seeds(1234, 0, 64, attempt=attempt), clip_seeds(1234, 64, 64, attempt=attempt),
                                clip_seeds(1234, 128, 2, attempt=attempt)])
        assert np.array_equal(whole, split)
        for c, s in enumerate(whole):
            vals[(c, attempt)] = int(s)
    assert len(set(vals.values())) == 130 * 6
    assert np.array_equal(clip_seeds(1234, 0, 4), clip_seeds(1234, 0, 4, attempt=0))
    assert not np.array_equal(clip_seeds(1234, 0, 4), clip_seeds(1235, 0, 4))


# ----------------------------------------------------------------------------------------------- compression_ratio
def hf_ratio(tokens, vocab):
    length = int(np.log2(vocab) / 8) + 1
    data = b"".join(int(t).to_bytes(length, "little") for t in tokens)
    return len(data) / len(zlib.compress(data))


def test_compression_ratio_matches_the_formula():
    vocab, eos = 51865, 50257
    rep = [1234] * 40
    assert compression_ratio(rep, vocab) == hf_ratio(rep, vocab) > 2.4
    rnd = np.random.default_rng(0).integers(0, 50000, size=40)
    assert compression_ratio(rnd, vocab) == hf_ratio(rnd, vocab) < 2.4
    # it stops at the first EOS (the pads after it, which may equal EOS, do not count)
    row = list(rnd[:12]) + [eos] + [eos] * 27
    assert compression_ratio(row, vocab, eos) == hf_ratio(rnd[:12], vocab)
    assert compression_ratio(row, vocab) == hf_ratio(row, vocab)
    assert compression_ratio([], vocab, eos) == 0.0
    assert compression_ratio([eos, 5, 6], vocab, eos) == 0.0
    assert int(np.log2(vocab) / 8) + 1 == 2 and int(np.log2(300) / 8) + 1 == 2 and int(np.log2(200) / 8) + 1 == 1
