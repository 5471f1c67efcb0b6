"""CPU: the semantics of per-clip prompts of different lengths, pinned on the numpy oracle, and
the pack / unpack helper.

The one sentence the GPU tests check — clip b of a ragged batch decodes exactly as clip b decoded alone with its
own prompt — is first checked on the restatement itself (tests/prompts_np.py: left-padded rows, per-row key window,
shifted positions, dead slots), which is the layout the kernels implement; then the restatement with either rule
switched off shows that the GPU tests' tolerances can tell a wrong implementation; then the condition the bf16 test
rests on is shown to hold on the reference alone."""
import functools

import numpy as np
import pytest

import prompts_np as PN
from oracle import whisper_np as W
from whisper_context_biasing_amd import prompts as P
from whisper_context_biasing_amd.config import get_dims
from whisper_context_biasing_amd.synth import synth_batch
from whisper_context_biasing_amd.weights import make_weights

TAU = 0.05          # tests/test_gpu_configs.py's margin gate
F32_LOGPROB_ATOL = 1e-3   # test_gpu_prompts.py's f32 end-to-end tolerance (test_gpu_logprobs.py's)


@functools.lru_cache(maxsize=None)
def case(size, recipe, seed):
    dims = get_dims(size)
    om = W.OracleModel.from_dims(dims, make_weights(dims, seed=seed, recipe=recipe))
    enc = om.encode(W.log_mel(synth_batch(5), dims.n_mel))
    return om, enc


@functools.lru_cache(maxsize=None)
def solo(size, recipe, seed):
    om, enc = case(size, recipe, seed)
    return PN.solo_decodes(om, enc, PN.fixed_prompts(), margins=True)


# ------------------------------------------------------------------------------------------------ the helper
def test_pack_layout():
    rows, lens = P.pack_prompts([[], [7], [1, 2, 3]], start_token=99, pad_token=5)
    assert rows.dtype == np.int32 and lens.dtype == np.int32
    assert lens.tolist() == [1, 2, 4]
    assert rows.tolist() == [[5, 5, 5, 99], [5, 5, 7, 99], [1, 2, 3, 99]]
    assert P.unpack_prompts(rows, lens) == [[], [7], [1, 2, 3]]
    # the generated columns behind the prompt do not disturb the unpacking
    seq = np.concatenate([rows, np.arange(6).reshape(3, 2)], axis=1)
    assert P.unpack_prompts(seq, lens) == [[], [7], [1, 2, 3]]


def test_pack_fixed_prompts_round_trip():
    prompts = PN.fixed_prompts()
    assert [len(p) for p in prompts] == PN.PROMPT_TOKENS and prompts[1] == [50360]
    rows, lens = P.pack_prompts(prompts, 50258, 50257)
    assert rows.shape == (5, 71) and lens.tolist() == [1, 2, 7, 64, 71]
    assert (rows[:, -1] == 50258).all() and (rows[0, :-1] == 50257).all() and not (rows[4] == 50257).any()
    assert P.unpack_prompts(rows, lens) == prompts


def test_nested_detection():
    assert P.is_nested([[1], []]) and P.is_nested(([1, 2], (3,))) and P.is_nested(np.zeros((2, 3), np.int64))
    assert not P.is_nested(None) and not P.is_nested([1, 2, 3]) and not P.is_nested(np.arange(3)) and not P.is_nested([])
    assert P.as_lists([np.arange(2), ()]) == [[0, 1], []]
    with pytest.raises(ValueError):
        P.pack_prompts([], 1, 0)
    with pytest.raises(ValueError):
        P.unpack_prompts(np.zeros((2, 1)), [1, 3])


# ------------------------------------------------------------------------------------------------ (a) semantics
def test_restatement_equals_the_solo_decodes():
    om, enc = case("micro", "diverse", 0)
    ids_s, lp_s, _ = solo("micro", "diverse", 0)
    ids, lp, rows, lens = PN.generate_ragged(om, enc, PN.fixed_prompts())
    err = np.abs(lp - lp_s).max()
    print(f"restatement vs solo: ids equal {np.array_equal(ids, ids_s)}, max |dlogprob| {err:.3e}")
    assert ids.shape == (5, PN.N_NEW) and np.array_equal(ids, ids_s)
    assert err < 1e-4, err
    assert rows.shape == (5, 71) and lens.tolist() == [1, 2, 7, 64, 71]


# ------------------------------------------------------------------------- (b) the GPU tests can tell a wrong one
@pytest.mark.parametrize("wrong", ["window", "shift"])
def test_wrong_variants_move_the_logprobs(wrong):
    """Without the key window (a live query also reads the dead slots' K/V) or without the shifted positions, the
    log-probs of every clip shorter than Pmax (rows 0-3) move by more than 0.03 = 30x the f32 tolerance the GPU
    test holds against the same oracle."""
    om, enc = case("micro", "diverse", 0)
    _, lp_s, _ = solo("micro", "diverse", 0)
    _, lp, _, _ = PN.generate_ragged(om, enc, PN.fixed_prompts(), window=wrong != "window", shift=wrong != "shift")
    moved = np.abs(lp - lp_s).max(axis=1)
    print(f"without the {wrong}: max |dlogprob| per row {np.round(moved, 4).tolist()}")
    assert (moved[:4] > 0.03).all(), moved
    assert 0.03 > 10 * F32_LOGPROB_ATOL


# ------------------------------------------------------------------------------ (c) the bf16 test's condition
def test_bf16_gate_condition_holds_on_the_reference():
    """tiny.en / margin / seed 1 with the fixed prompts: every one of the 60 oracle margins is >= TAU, so
    gated_equal in the bf16 GPU test checks 60 / 60 tokens whatever the implementation does."""
    _, _, mg = solo("tiny.en", "margin", 1)
    print(f"tiny.en margin s1 with prompts: min margin {mg.min():.3f}")
    assert mg.shape == (5, PN.N_NEW) and (mg >= TAU).all(), mg.min()
