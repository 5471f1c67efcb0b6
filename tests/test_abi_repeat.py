"""CPU: the repeat-rule entry points are declared in include/wcb.h with the stated arity, exported by libwcb.so and
bound in the ctypes table; the declaration they are modelled on is textually unchanged; the struct has the stated
fields (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from whisper_context_biasing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wcb.h")
NEW = {"wcb_set_repeat_rules": 2, "wcb_repeat_rules_apply_host": 5, "wcb_op_lm_head_repeat": 16}
UNCHANGED = {
    "wcb_set_token_rules": "wcb_handle*, const wcb_token_rules*",
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


def test_header_declares_the_struct():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} wcb_repeat_rules;", src)
    assert m, "wcb_repeat_rules"
    names = re.findall(r"(\w+)\s*;", m.group(1))
    assert names == ["repetition_penalty", "no_repeat_ngram_size"]
    assert [n for n, _ in _lib.WcbRepeatRules._fields_] == names
    assert C.sizeof(_lib.WcbRepeatRules) == 8


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_existing_signatures_are_unchanged(name):
    assert re.sub(r"\s+", " ", declarations()[name]).strip() == UNCHANGED[name]


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (wcb_[a-z_0-9]+)$", out, flags=re.M))
    assert not [s for s in NEW if s not in exported]
    lib = _lib.load()
    # null handles / pointers are refused with a status before any device is touched
    assert lib.wcb_set_repeat_rules(None, None) == -1
    r = _lib.WcbRepeatRules(1.2, 2)
    assert lib.wcb_set_repeat_rules(None, C.byref(r)) == -1
    assert lib.wcb_repeat_rules_apply_host(C.byref(r), 0, None, 0, None) == -1
    assert lib.wcb_op_lm_head_repeat(_lib.WCB_F32, None, None, 1, 8, 64, 0, C.byref(r), 0, None, 1, None, None, 8, None, None) == -1
