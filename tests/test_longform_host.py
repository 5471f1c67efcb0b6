"""CPU: the host side of long-form transcription.

1. whisper_context_biasing_amd.longform's segment / seek rule and previous-token prompts equal HF's own
   `_retrieve_segment` and `_pad_to_max_length(skip_ending_double_timestamps=True, cut_off_length=223)` on every
   sequence of tests/golden/longform_rules.npz: segments, times, segment_offset, prompts — exactly.
2. tests/longform_np.py, the numpy restatement of the whole loop, equals the reference class's long-form generate()
   (tests/golden/longform_micro_diverse_s0.npz): ids, seeks and segment times, conditioning off and on, both recipes —
   and the oracle's own margins satisfy the fixture's condition at every step of every window.
3. The numpy long log-mel equals HF's extractor in long mode (tests/golden/longform_mel.npz).
4. The refusals raise ValueError; the skip rule and the loop state."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longform_np as LN  # noqa: E402
from whisper_context_biasing_amd import longform as LF  # noqa: E402
from whisper_context_biasing_amd.config import get_dims, no_speech_token_id, start_of_prev_token_id, timestamp_ids  # noqa: E402

RULES = np.load(os.path.join(LN.GOLDEN, "longform_rules.npz"))
E2E = np.load(os.path.join(LN.GOLDEN, "longform_micro_diverse_s0.npz"))


def test_special_ids():
    for size, (sop, nsp) in {"tiny.en": (50360, 50361), "micro": (50361, 50362), "small": (50361, 50362), "large-v3": (50362, 50363)}.items():
        d = get_dims(size)
        assert (start_of_prev_token_id(d), no_speech_token_id(d)) == (sop, nsp)
        assert no_speech_token_id(d) == timestamp_ids(d)[1] - 1


def test_segment_rule_equals_hf():
    ts0 = int(RULES["timestamp_begin"])
    names = [str(n) for n in RULES["names"]]
    assert {"no_timestamp", "no_pair_last_is_ts0", "no_pair_last_above", "one_pair_open_tail", "single_timestamp_ending",
            "ending_in_pair", "short_last_window_no_pair"} <= set(names)
    assert int(RULES["n_cases"]) == len(names) >= 12 + 40
    for k, name in enumerate(names):
        seek, nf, off = (int(v) for v in RULES[f"k{k}_seek_nf_off"])
        segs, got_off = LF.retrieve_segments(RULES[f"k{k}_seq"], seek, nf, ts0)
        assert got_off == off, (name, got_off, off)
        assert [len(s[2]) for s in segs] == RULES[f"k{k}_lens"].tolist(), name
        assert [t for s in segs for t in s[2]] == RULES[f"k{k}_tokens"].tolist(), name
        assert np.array_equal(np.asarray([s[0] for s in segs]), RULES[f"k{k}_start"]), (name, segs, RULES[f"k{k}_start"])
        assert np.array_equal(np.asarray([s[1] for s in segs]), RULES[f"k{k}_end"]), (name, segs, RULES[f"k{k}_end"])


def test_previous_token_prompts_equal_hf():
    ts0, sop, cut = int(RULES["timestamp_begin"]), int(RULES["prev_sot"]), int(RULES["cut_off_length"])
    longest = 0
    for j in range(int(RULES["n_hist"])):
        segs = []
        for k in RULES[f"h{j}_cases"]:
            lens, toks = RULES[f"k{k}_lens"], RULES[f"k{k}_tokens"].tolist()
            o = 0
            for n in lens:
                segs.append(toks[o:o + n])
                o += n
        longest = max(longest, sum(len(s) for s in segs))
        got = LF.window_prompt(segs, condition_on_prev_tokens=True, prev_sot=sop, timestamp_begin=ts0, n_text_ctx=448)
        assert got == RULES[f"h{j}_prompt"].tolist(), j
        assert len(got) <= cut + 1
    assert longest > cut   # one history is cut off
    assert LF.window_prompt([], condition_on_prev_tokens=True, prev_sot=sop, timestamp_begin=ts0, n_text_ctx=448) == []
    assert LF.window_prompt([[1, 2]], condition_on_prev_tokens=False, prev_sot=sop, timestamp_begin=ts0, n_text_ctx=448) == []
    # a user prompt: alone without conditioning; as the head with "all-segments"; as a pseudo-segment with "first-segment"
    kw = dict(prev_sot=sop, timestamp_begin=ts0, n_text_ctx=448)
    assert LF.window_prompt([[1, 2]], condition_on_prev_tokens=False, prompt_ids=[sop, 9], **kw) == [sop, 9]
    assert LF.window_prompt([[1, 2]], condition_on_prev_tokens=True, prompt_ids=[sop, 9], prompt_condition_type="all-segments",
                            **kw) == [sop, 9, 1, 2]
    st = LF.LongFormState([100], eos=50257, pad=50257, condition_on_prev_tokens=True, prompt_ids=[sop, 9, 10], **kw)
    assert st.prompts([0]) == [[sop, 9, 10]]
    st.update([0], [[ts0, 5, ts0 + 3, ts0 + 3, 50257, 50257]])
    assert st.prompts([0]) == [[sop, 9, 10, ts0, 5, ts0 + 3]] and st.seek == [6] and st.sequences().tolist() == [[ts0, 5, ts0 + 3, ts0 + 3]]


def test_strip_and_skip_and_state():
    eos = pad = 50257
    assert LF.strip_window([5, 6, eos, pad, pad], eos, pad) == [5, 6]
    assert LF.strip_window([5, 6, 7], eos, pad) == [5, 6, 7]
    assert LF.strip_window([5, 6, 9, 3, 3], 9, 3) == [5, 6]
    assert LF.should_skip(-1.5, 0.7, -1.0, 0.6) and not LF.should_skip(-0.5, 0.7, -1.0, 0.6)
    assert not LF.should_skip(-1.5, 0.5, -1.0, 0.6) and not LF.should_skip(-1.5, 0.7, -1.0, None)
    ts0 = 50364
    st = LF.LongFormState([3337, 900], eos=eos, pad=pad, timestamp_begin=ts0, prev_sot=50361, n_text_ctx=448,
                          logprob_threshold=-1.0, no_speech_threshold=0.6)
    assert st.active() == [0, 1]
    s, n = st.windows([0, 1])
    assert s.tolist() == [0, 0] and n.tolist() == [3000, 900]
    st.update([0, 1], [[ts0, 5, ts0 + 100, ts0 + 100, 7, eos], [ts0, 5, eos, pad, pad, pad]], [-0.2, -2.0], [0.1, 0.9])
    assert st.seek == [200, 900] and st.active() == [0]          # clip 1 skipped: no segments, seek past the window
    assert st.segments[1] == [] and st.skipped == [[False], [True]] and len(st.segments[0]) == 1
    assert st.seeks == [[0], [0]] and st.windows([0])[1].tolist() == [3000]
    with pytest.raises(ValueError):
        LF.LongFormState([0], eos=eos, pad=pad, timestamp_begin=ts0, prev_sot=50361, n_text_ctx=448)


def test_refusals():
    for kw in (dict(temperature=(0.0, 0.2)), dict(temperature=0.4), dict(num_beams=2),
               dict(return_token_timestamps=True, condition_on_prev_tokens=True), dict(prompt_condition_type="every-segment"),
               dict(prompt_ids=[1], prompt_condition_type="all-segments")):
        with pytest.raises(ValueError):
            LF.check_args(**kw)
    LF.check_args()
    LF.check_args(condition_on_prev_tokens=True, prompt_ids=[1], prompt_condition_type="all-segments")


def test_numpy_long_log_mel_equals_hf():
    MEL_SLICES, mel_clips = LN.MEL_SLICES, LN.mel_clips
    g = np.load(os.path.join(LN.GOLDEN, "longform_mel.npz"))
    clips = mel_clips()
    for n_mel in (80, 128):
        m, frames = LN.log_mel_long(clips, n_mel)
        assert m.shape == (2, n_mel, 3337) and frames.tolist() == g[f"max_frames_{n_mel}"].tolist() == [3337, 1250]
        for i in range(2):
            got = np.concatenate([m[i][:, s] for s in MEL_SLICES[i]], axis=1)
            assert np.abs(got - g[f"mel{n_mel}_clip{i}_slices"]).max() < 2e-5


@pytest.mark.parametrize("recipe", ["diverse", "margin"])
@pytest.mark.parametrize("cond", [False, True])
def test_restatement_equals_reference(recipe, cond):
    ref = LN.e2e_reference(cond, recipe)
    n_seg = 0
    for b in range(len(LN.CLIP_SECONDS)):
        st, windows = ref[b]
        key = f"{recipe}_cond{int(cond)}_clip{b}_"
        for w in windows:   # the condition on the fixture: no step is excluded from the f32 comparisons
            assert w["top2"].min() >= LN.MARGIN and w["rule5"].min() >= LN.MARGIN
        assert np.array_equal(st.sequences()[0], E2E[key + "sequence"])
        assert st.seeks[0] == E2E[key + "seeks"].tolist()
        assert [len(s[2]) for s in st.segments[0]] == E2E[key + "seg_lens"].tolist()
        assert np.array_equal(np.asarray([s[0] for s in st.segments[0]]), E2E[key + "seg_start"])
        assert np.array_equal(np.asarray([s[1] for s in st.segments[0]]), E2E[key + "seg_end"])
        n_seg += len(st.segments[0])
    if recipe == "diverse":   # timestamp-driven seeks, and with conditioning prompts that really carry previous text
        assert n_seg >= 30 and ref[0][0].seeks[0][1] not in (0, 3000)
        if cond:
            assert len(ref[0][1][1]["prompt"]) > 1 and ref[0][1][1]["prompt"][0] == start_of_prev_token_id(LN.e2e_case()["dims"])
    else:                     # the no-pair branch: window-length segments
        assert ref[0][0].seeks[0] == [0, 3000, 6000]
