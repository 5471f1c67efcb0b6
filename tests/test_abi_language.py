"""CPU: the language entry points are declared in include/wcb.h with the stated arity, exported by libwcb.so and bound
in the ctypes table; the declarations they sit beside are textually unchanged; argument errors come back as a status
before any device is touched (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from whisper_context_biasing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wcb.h")
NEW = {"wcb_detect_language": 9, "wcb_generate_lang": 15, "wcb_decode_begin_lang": 12, "wcb_op_lang_head": 14}
UNCHANGED = {
    "wcb_generate_prompted": "wcb_handle*, const float* mel, int B, const wcb_gen_cfg*, const wcb_sample_cfg*, "
                             "const wcb_bias*, const wcb_bias_batch*, const int32_t* prompts, int prompt_ld, "
                             "const int32_t* prompt_len, int32_t* out_ids, float* out_logprobs, int32_t* out_steps, "
                             "void* stream",
    "wcb_decode_begin_prompted": "wcb_handle*, const void* enc, int B, const int32_t* prompts, int prompt_ld, "
                                 "const int32_t* prompt_len, float bias_boost, int min_new_tokens, wcb_state** out, "
                                 "void* stream",
    "wcb_op_lm_head_rules": "int dtype, const void* A, const void* W, int M, int V, int K, int walkers, "
                            "const wcb_token_rules* rules, int eos, const int32_t* generated, int gen_ld, "
                            "const int32_t* lens, float* logits, long ld, int32_t* next_ids, void* stream",
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


def test_header_declares_the_config():
    src = open(HEADER).read()
    m = re.search(r"typedef struct \{([^}]*)\} wcb_lang_cfg;", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert m, "wcb_lang_cfg"
    names = re.findall(r"(\w+)\s*[;,]", m.group(1))
    assert names == ["lang_begin", "n_lang", "candidates", "column_from_end", "out_ids", "out_probs"]
    assert [n for n, _ in _lib.WcbLangCfg._fields_] == names


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_existing_signatures_are_unchanged(name):
    assert re.sub(r"\s+", " ", declarations()[name]) == UNCHANGED[name]


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (wcb_[a-z_0-9]+)$", out, flags=re.M))
    assert not [s for s in NEW if s not in exported]
    lib = _lib.load()
    # null handles / pointers are refused with a status before any device is touched
    assert lib.wcb_detect_language(None, None, 1, 50259, 99, None, None, None, None) == -1
    assert lib.wcb_generate_lang(None, None, 1, None, None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert lib.wcb_decode_begin_lang(None, None, 1, 1, None, 1, None, None, 0.0, 0, None, None) == -1
    # the op checks its range and its candidates on the host, before the first launch: the operands are never read
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data

    def op(V, lang_begin, n_lang, cand=None, M=1, K=8):
        return lib.wcb_op_lang_head(_lib.WCB_F32, p, p, M, V, K, lang_begin, n_lang,
                                    cand.ctypes.data if cand is not None else None, p, None, p, V, None)

    assert op(2200, 2150, 99) == -1                              # the range ends past the vocabulary
    assert op(2200, -1, 99) == -1                                # ... or starts before it
    assert op(2200, 699, 0) == -1 and op(2200, 699, 114) == -1   # n_lang outside [1, 113]
    msg = lib.wcb_last_error(None).decode()
    assert "n_lang" in msg, msg
    assert op(2200, 699, 99, np.zeros(4, dtype=np.uint32)) == -1  # an empty candidate set
    assert "names no language" in lib.wcb_last_error(None).decode()
    bits = np.zeros(4, dtype=np.uint32)
    bits[3] = 1 << 4                                             # bit 100: outside n_lang = 99, so still empty
    assert op(2200, 699, 99, bits) == -1
    assert op(2200, 699, 99, M=65) == -1 and op(2200, 699, 99, K=2561) == -1
    assert C.sizeof(_lib.WcbLangCfg) == 40
