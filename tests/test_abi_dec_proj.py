"""CPU: the decode-projection entry points (wcb_op_embed, wcb_op_dec_proj) are declared in include/wcb.h with the
stated arity, exported by libwcb.so and bound in the ctypes table, the descriptor struct matches field for field,
the wcb_op_* declarations they sit beside are textually unchanged, and null pointers are refused before any device
call (no compute: there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from whisper_context_biasing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wcb.h")
NEW = {"wcb_op_embed": 17, "wcb_op_dec_proj": 2}
UNCHANGED = {
    "wcb_op_gemm": "int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int act, "
                   "const float* resid, void* out, int out_f32, void* stream",
    "wcb_op_gemm_kernel": "int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int act, "
                          "const float* resid, void* out, int out_f32, int kernel, void* stream",
    "wcb_op_gemm_ln": "int dtype, const float* X, const float* ln_w, const float* ln_b, const float* stats, "
                      "const void* W, int M, int N, int K, const float* bias, int act, void* out, int out_f32, "
                      "void* stream",
    "wcb_op_lm_head_lse": "int dtype, const void* A, const void* W, int M, int V, int K, int walkers, float* logits, long ld, "
                          "float* lse, int32_t* argmax, void* stream",
    "wcb_op_layernorm": "int dtype, const float* x, const float* w, const float* b, void* y, int M, int d, "
                        "void* stream",
    "wcb_op_attention_decode": "int dtype, const void* q, const void* k, const void* v, void* o, int B, int H, "
                               "int Sk, int nsplit, int variant, void* stream",
    "wcb_op_cross_attention_enc": "int dtype, const void* q, const void* enc, const void* wkt, const void* wv, "
                                  "const float* bv, void* o, int B, int H, int S, int nsplit, int variant, void* stream",
}


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declarations():
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(wcb_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", _source(), flags=re.S)}


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_declares_entry_point(name):
    decl = declarations()
    assert name in decl, name
    assert len(decl[name].split(",")) == NEW[name], decl[name]
    assert len(_lib.SIGNATURES[name][1]) == NEW[name]


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_existing_op_signatures_are_unchanged(name):
    assert re.sub(r"\s+", " ", declarations()[name]) == UNCHANGED[name]


def test_descriptor_matches_the_header_field_for_field():
    body = re.search(r"typedef struct \{([^}]*)\} wcb_dec_proj;", _source()).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        head, *more = [s.strip() for s in stmt.split(",")]
        ctype, first = head.rsplit(" ", 1) if "*" not in head else (head[:head.rindex("*") + 1], head[head.rindex("*") + 1:])
        for nm in [first] + more:
            fields.append((nm.strip(), "*" in ctype))
    got = [(n, t is C.c_void_p or t == C.POINTER(C.c_int32)) for n, t in _lib.WcbDecProj._fields_]
    assert got == fields
    enums = dict(re.findall(r"(WCB_(?:PROJ|PATH)_[A-Z_]+) = (\d+)", _source()))
    for k, v in enums.items():
        assert getattr(_lib, k[4:]) == int(v), k
    assert len(enums) == 13


def test_library_exports_and_refuses_null_pointers():
    _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (wcb_[a-z_0-9]+)$", out, flags=re.M))
    assert not [s for s in NEW if s not in exported]
    lib = _lib.load()
    assert lib.wcb_op_embed(_lib.WCB_BF16, None, None, None, None, None, 4, 64, 10, 8, 1, None, None, None, None, 16, None) == -1
    assert lib.wcb_op_dec_proj(None, None) == -1
    for kind in range(6):
        for path in range(7):
            p = _lib.WcbDecProj(kind=kind, path=path, dtype=_lib.WCB_BF16, M=5, N=768, K=768)
            assert lib.wcb_op_dec_proj(C.byref(p), None) == -1, (kind, path)
    # out-of-range selectors and shapes
    for bad in (dict(kind=6), dict(path=7), dict(dtype=3), dict(M=0), dict(N=24), dict(K=100)):
        kw = dict(kind=0, path=0, dtype=_lib.WCB_BF16, M=5, N=768, K=768)
        kw.update(bad)
        assert lib.wcb_op_dec_proj(C.byref(_lib.WcbDecProj(**kw)), None) == -1, bad
