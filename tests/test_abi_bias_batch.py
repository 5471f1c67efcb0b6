"""CPU: the per-utterance bias-list entry points are declared in include/wcb.h, exported by libwcb.so and
bound in the ctypes table with the declared arity (no compute calls: there is no GPU here)."""
import os
import re
import subprocess

import pytest

from whisper_context_biasing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wcb.h")
NEW = {"wcb_bias_batch_create": 7, "wcb_bias_batch_destroy": 1, "wcb_bias_batch_num_states": 2,
       "wcb_generate_biased": 10, "wcb_decode_bias_batch": 3, "wcb_debug_counter": 3}


def declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(wcb_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_declares_entry_point(name):
    decl = declarations()
    assert name in decl, name
    assert len(decl[name].split(",")) == NEW[name], decl[name]
    assert len(_lib.SIGNATURES[name][1]) == NEW[name]


def test_existing_signatures_are_unchanged():
    decl = declarations()
    assert re.sub(r"\s+", " ", decl["wcb_generate"]) == (
        "wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias, "
        "const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream")
    assert re.sub(r"\s+", " ", decl["wcb_decode_step"]) == (
        "wcb_handle* h, wcb_state* st, const wcb_bias* bias, int32_t* next_ids, float* scores, void* stream")


def test_library_exports_the_entry_points():
    _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (wcb_[a-z_0-9]+)$", out, flags=re.M))
    assert not [s for s in NEW if s not in exported]
    lib = _lib.load()
    # host-only calls that need no device: null arguments are refused with a status, and a null batch is inert
    assert lib.wcb_debug_counter(None, b"graph_captures", None) == -1
    assert lib.wcb_bias_batch_num_states(None, -1) == 0
    lib.wcb_bias_batch_destroy(None)
