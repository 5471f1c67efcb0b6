"""Long-form cost per 30 s window against what a caller had before it: whisper-small, bf16, 16 recordings of 120 s, EOS
masked so every window decodes --tokens tokens, the four windows at fixed 30 s strides (seek 0, 3000, 6000, 9000), every
clip with a prompt of its own (lengths uniform in --min-prompt .. --max-prompt, as condition_on_prev_tokens gives).
Interleaved round by round, in a new seeded order every round; per figure the median of --reps timed rounds (min, max beside it) after --warmup rounds.

  front_long      wcb_log_mel_long of the 16 recordings once (a quarter of it charged to each window) + the device
                  window cut + the encoder (wcb_encode_windows)
  front_sliced    the same long features sliced on the host side ([:, :, s:s+3000].contiguous()) + wcb_encode (its
                  mel_to_conv_input): the device cut against host slicing
  front_base      what the parent commit offers: the PCM cut at 30 s, wcb_log_mel per window + wcb_encode
  call_long       one window's whole decode call from the long features (cut + encoder + prefill + decode, no-speech probe
                  on): wcb_generate_windows
  call_base       generate() on the window's own 30 s features with the same prompts, timestamps and log-probs

decode_long / decode_base = the call minus that path's cut + encoder. Prints one JSON line.

  python tools/longform_bench.py [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time
from dataclasses import replace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisper_context_biasing_amd import request as RQ  # noqa: E402
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB, _WindowBatch  # noqa: E402
from whisper_context_biasing_amd.synth import synth_clip  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="small")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=int, default=120)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--min-prompt", type=int, default=100)
    ap.add_argument("--max-prompt", type=int, default=224)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of fewer calls is not reported)")
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    B, nwin = a.batch, a.seconds // 30
    pcm = torch.from_numpy(np.stack([synth_clip(300 + b, n_samples=a.seconds * 16000) for b in range(B)])).cuda()
    rng = np.random.RandomState(5)
    prompts = [rng.randint(300, 20000, n).tolist() for n in rng.randint(a.min_prompt, a.max_prompt + 1, B)]
    rows = list(range(B))
    req = RQ.resolve(dims, m.generation_config, B, max_length=a.tokens, min_new_tokens=a.tokens, prompt_ids=prompts,
                     output_logprobs=True, return_timestamps=True)
    gen_kw = dict(max_length=a.tokens, min_new_tokens=a.tokens, prompt_ids=prompts, output_logprobs=True, return_timestamps=True)
    feats, _ = m.log_mel_long(pcm)
    T = feats.shape[2]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        m.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def window(w):
        return [w * 3000] * B, [3000] * B

    work = {
        "log_mel_long": lambda w: m.log_mel_long(pcm),
        "cut_encode": lambda w: m.encode_windows(feats, rows, *window(w)),
        "slice_encode": lambda w: m.encode(feats[:, :, w * 3000:(w + 1) * 3000].contiguous()),
        "base_mel_encode": lambda w: m.encode(m.log_mel(pcm[:, w * 480000:(w + 1) * 480000])),
        "call_long": lambda w: m._decode(_WindowBatch(feats, T, rows, *window(w)), replace(req)),
        "call_base": lambda w: m.generate(feats[:, :, w * 3000:(w + 1) * 3000].contiguous(), **gen_kw),
    }
    times = {k: [] for k in work}
    for _ in range(max(a.warmup, 2)):
        for k, f in work.items():
            f(0)
    m.synchronize()
    names = list(work)
    for r in range(a.reps):   # a new order every round: no workload always runs behind the same one (a call that follows
        # a short one starts on a cooler chip: with a fixed order the cut measured 0.45 ms above the host slice)
        for k in np.random.RandomState(100 + r).permutation(names):
            times[k].append(timed(lambda: work[k](r % nwin))[0])
    ids_long = work["call_long"](1).sequences
    ids_base = work["call_base"](1).sequences
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"model": a.model, "batch": B, "seconds": a.seconds, "tokens": a.tokens, "dtype": a.dtype, "reps": a.reps,
           "windows_per_recording": nwin, "prompt_tokens": [min(map(len, prompts)), max(map(len, prompts))],
           "long_base_token_agreement": round(float((ids_long == ids_base).float().mean()), 4)}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    res["front_long_ms_per_window"] = round(med["log_mel_long"] / nwin + med["cut_encode"], 3)
    res["front_sliced_ms_per_window"] = round(med["log_mel_long"] / nwin + med["slice_encode"], 3)
    res["front_base_ms_per_window"] = round(med["base_mel_encode"], 3)
    res["decode_long_ms_per_window"] = round(med["call_long"] - med["cut_encode"], 3)
    res["decode_base_ms_per_window"] = round(med["call_base"] - med["slice_encode"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
