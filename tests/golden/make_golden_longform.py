"""Generate the long-form fixtures by running the REFERENCE stack itself (survey container only), as make_golden.py
does: HF's `WhisperGenerationMixin` static rules, HF's `WhisperFeatureExtractor` in long mode and the reference model
class's long-form generate(). Data only is stored (inputs are regenerated from seeds):

  longform_rules.npz              _retrieve_segment / _pad_to_max_length on crafted and random token sequences
  longform_mel.npz                the extractor with truncation=False, padding="longest" on two clips (33.37 s, 12.5 s)
  longform_micro_diverse_s0.npz   generate(return_timestamps=True, return_segments=True, temperature=0.0) per clip
                                  (B = 1 calls), conditioning off and on, `diverse` and `margin` recipes

Run:  python tests/golden/make_golden_longform.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import longform_np as LN  # noqa: E402
from make_golden import ref_model  # noqa: E402
from whisper_context_biasing_amd.config import get_dims, start_of_prev_token_id, timestamp_ids  # noqa: E402

TS0, EOS, PAD, SOP = 50364, 50257, 50257, 50361
CUT_OFF = 223


# ------------------------------------------------------------------------------------------------- rules
def crafted_sequences():
    """(name, ids, seek, seek_num_frames): one per branch of _retrieve_segment"""
    t = lambda k: TS0 + k   # noqa: E731
    return [
        ("no_timestamp", [11, 12, 13], 0, 3000),
        ("no_pair_last_is_ts0", [t(0), 11, 12], 600, 3000),
        ("no_pair_last_above", [t(0), 11, 12, t(40), 13], 600, 3000),
        ("one_pair_open_tail", [t(0), 11, 12, t(100), t(100), 13, 14], 0, 3000),
        ("single_timestamp_ending", [t(0), 11, t(100), t(100), 13, 14, t(250)], 1234, 3000),
        ("ending_in_pair", [t(0), 11, t(100), t(100), 13, 14, t(250), t(250)], 1234, 3000),
        ("two_pairs_open_tail", [t(5), 11, t(100), t(100), 13, t(180), t(180), 15, 16, 17], 77, 3000),
        ("short_last_window_no_pair", [t(0), 11, 12], 6000, 337),
        ("short_last_window_single_ending", [t(0), 11, t(10), t(10), 12, t(16)], 6000, 337),
        ("short_last_window_pair", [t(0), 11, t(10), t(10)], 6000, 337),
        ("one_token", [t(3)], 0, 3000),
        ("only_a_pair_after_text", [t(0), 5, t(7), t(7)], 3, 900),
    ]


def random_sequence(g):
    """a sequence the timestamp grammar can produce: a timestamp first, text runs, single or doubled timestamps, times
    never decreasing and growing across a text run"""
    cur, seq = int(g.integers(0, 30)), []
    seq.append(TS0 + cur)
    for _ in range(int(g.integers(0, 7))):
        seq += [int(v) for v in g.integers(0, EOS, int(g.integers(1, 5)))]
        cur += int(g.integers(1, 200))
        if cur > 1500:
            break
        seq.append(TS0 + cur)
        u = g.random()
        if u < 0.6:
            seq.append(TS0 + cur)
        elif u < 0.8:
            break
    if g.random() < 0.4:
        seq += [int(v) for v in g.integers(0, EOS, int(g.integers(1, 4)))]
    return seq


def rules_fixture():
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as G, _pad_to_max_length
    g = np.random.default_rng(20)
    cases = crafted_sequences()
    for k in range(40):
        nf = int(g.choice([3000, 3000, 3000, 1700, 337]))
        cases.append((f"random{k}", random_sequence(g), int(g.integers(0, 9000)), nf))
    out = {"n_cases": np.int64(len(cases)), "names": np.array([c[0] for c in cases]), "timestamp_begin": np.int64(TS0),
           "prev_sot": np.int64(SOP), "cut_off_length": np.int64(CUT_OFF)}
    all_tokens = []
    for k, (_, seq, seek, nf) in enumerate(cases):
        seek_t = torch.tensor([seek], dtype=torch.long)
        segs, off = G._retrieve_segment(
            seek_sequence=torch.tensor(seq, dtype=torch.long), seek_outputs=[None], time_offset=seek_t.to(torch.float64) * 0.02 / 2,
            timestamp_begin=TS0, seek_num_frames=torch.tensor([nf], dtype=torch.long), time_precision=0.02,
            time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0, return_token_timestamps=False,
            decoder_input_ids=torch.zeros(1, 1, dtype=torch.long))
        out[f"k{k}_seq"] = np.asarray(seq, dtype=np.int64)
        out[f"k{k}_seek_nf_off"] = np.asarray([seek, nf, int(off)], dtype=np.int64)
        out[f"k{k}_start"] = np.asarray([float(s["start"]) for s in segs], dtype=np.float64)
        out[f"k{k}_end"] = np.asarray([float(s["end"]) for s in segs], dtype=np.float64)
        out[f"k{k}_lens"] = np.asarray([len(s["tokens"]) for s in segs], dtype=np.int64)
        out[f"k{k}_tokens"] = np.concatenate([s["tokens"].numpy() for s in segs]).astype(np.int64)
        all_tokens.append([s["tokens"] for s in segs])
    # previous-token prompts: the segments of several cases in a row as one clip's history; the last one longer than 223
    histories = [[0], [3], [5], [4, 5, 6], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], list(range(12, 52)), list(range(52))]
    out["n_hist"] = np.int64(len(histories))
    for j, hist in enumerate(histories):
        segs = [{"tokens": tk} for k in hist for tk in all_tokens[k]]
        prev = _pad_to_max_length([segs], PAD, device="cpu", padding_side="left", padding="longest",
                                  bos_token_tensor=torch.tensor([SOP]), cut_off_length=CUT_OFF,
                                  skip_ending_double_timestamps=True, timestamp_begin=TS0)
        out[f"h{j}_cases"] = np.asarray(hist, dtype=np.int64)
        out[f"h{j}_prompt"] = prev[0].numpy().astype(np.int64)
    n_long = sum(len(out[f"k{k}_tokens"]) for k in histories[-1])
    assert n_long > CUT_OFF, n_long
    np.savez_compressed(os.path.join(HERE, "longform_rules.npz"), **out)
    print("longform_rules.npz:", len(cases), "sequences,", len(histories), "histories, longest", n_long, "tokens")


# --------------------------------------------------------------------------------------------------- mel
def mel_fixture():
    from transformers import WhisperFeatureExtractor
    clips = LN.mel_clips()
    out = {}
    for n_mel in (80, 128):
        fe = WhisperFeatureExtractor(feature_size=n_mel)
        f = fe(clips, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="np")
        m, mask = f["input_features"], f["attention_mask"]
        assert m.shape == (2, n_mel, 3337), m.shape
        out[f"max_frames_{n_mel}"] = mask.sum(-1).astype(np.int64)
        mine, frames = LN.log_mel_long(clips, n_mel)
        assert np.array_equal(frames, out[f"max_frames_{n_mel}"]) and np.abs(mine - m).max() < 2e-5, np.abs(mine - m).max()
        for i in range(2):
            out[f"mel{n_mel}_clip{i}_slices"] = np.concatenate([m[i][:, s] for s in LN.MEL_SLICES[i]], axis=1)
            out[f"mel{n_mel}_clip{i}_stats"] = np.array(
                [m[i].sum(dtype=np.float64), np.abs(m[i]).sum(dtype=np.float64), m[i].max(), m[i].min()])
            # the first 30 s window's own statistics: a per-window clamp would leave another minimum there
            out[f"mel{n_mel}_clip{i}_first_window_min_max"] = np.array([m[i][:, :3000].min(), m[i][:, :3000].max()])
    np.savez_compressed(os.path.join(HERE, "longform_mel.npz"), **out)
    print("longform_mel.npz written; first-window (min, max) of clip 0:", out["mel80_clip0_first_window_min_max"],
          "whole clip (max, min):", out["mel80_clip0_stats"][2:])


# ------------------------------------------------------------------------------------------- end to end
def run_reference(m, dims, feats, max_frames, cond, suppress, begin):
    from transformers import GenerationConfig
    ts0, no_ts = timestamp_ids(dims)
    gc = GenerationConfig(max_new_tokens=LN.MAX_NEW, pad_token_id=dims.pad_token_id, eos_token_id=dims.eos_token_id,
                          decoder_start_token_id=dims.decoder_start_token_id, use_cache=True)
    gc.no_timestamps_token_id = no_ts
    gc.prev_sot_token_id = start_of_prev_token_id(dims)
    gc.max_initial_timestamp_index = LN.MAX_INIT_INDEX
    gc.suppress_tokens = list(suppress)
    gc.begin_suppress_tokens = list(begin)
    m.generation_config = gc
    m.config.suppress_tokens = None
    m.config.begin_suppress_tokens = None
    m.config.forced_decoder_ids = None
    seeks = []
    x = torch.from_numpy(feats[None, :, :max_frames].copy())
    with torch.no_grad():
        out = m.generate(input_features=x, attention_mask=torch.ones(1, max_frames, dtype=torch.long), return_timestamps=True,
                         return_segments=True, temperature=0.0, condition_on_prev_tokens=cond, logprob_threshold=None,
                         compression_ratio_threshold=None, no_speech_threshold=None,
                         monitor_progress=lambda p: seeks.append(int(p[0, 0])))
    segs = out["segments"][0]
    return dict(sequence=out["sequences"][0].numpy().astype(np.int64), seeks=np.asarray(seeks, dtype=np.int64),
                seg_start=np.asarray([float(s["start"]) for s in segs], dtype=np.float64),
                seg_end=np.asarray([float(s["end"]) for s in segs], dtype=np.float64),
                seg_lens=np.asarray([len(s["tokens"]) for s in segs], dtype=np.int64))


def e2e_fixture():
    out = {}
    for recipe, seed in (("diverse", 0), ("margin", 0)):
        c = LN.e2e_case(recipe, seed)
        dims = c["dims"]
        m = ref_model(dims, c["sd"])
        for cond in (False, True):
            ref = LN.e2e_reference(cond, recipe, seed)
            for b in range(len(LN.CLIP_SECONDS)):
                r = run_reference(m, dims, c["feats"][b], int(c["max_frames"][b]), cond, c["suppress"], c["begin"])
                st, windows = ref[b]
                top2 = min(float(w["top2"].min()) for w in windows)
                rule5 = min(float(w["rule5"].min()) for w in windows)
                print(f"{recipe} cond={int(cond)} clip{b}: {len(r['seg_lens'])} segments, seeks {r['seeks'].tolist()}, "
                      f"oracle min top-2 margin {top2:.4g}, min rule-5 margin {rule5:.4g}", flush=True)
                # the condition on the fixture: the reference alone resolves every step at the f32 device bound
                assert top2 >= LN.MARGIN and rule5 >= LN.MARGIN, "change the clip's seed or length"
                assert np.array_equal(st.sequences()[0], r["sequence"]), (st.sequences()[0], r["sequence"])
                assert st.seeks[0] == r["seeks"].tolist(), (st.seeks[0], r["seeks"])
                for k, v in r.items():
                    out[f"{recipe}_cond{int(cond)}_clip{b}_{k}"] = v
    out["meta"] = np.array([str(dict(size="micro", seed=0, clip_seconds=LN.CLIP_SECONDS, clip_seeds=LN.CLIP_SEEDS,
                                     max_new_tokens=LN.MAX_NEW, max_initial_timestamp_index=LN.MAX_INIT_INDEX))])
    np.savez_compressed(os.path.join(HERE, "longform_micro_diverse_s0.npz"), **out)
    print("longform_micro_diverse_s0.npz written")


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["rules", "mel", "e2e"]
    if "rules" in which:
        rules_fixture()
    if "mel" in which:
        mel_fixture()
    if "e2e" in which:
        e2e_fixture()
