"""Per-clip prompts of different lengths against the alternatives a caller had before them: whole-call time of
generate() (front end excluded: the mel is precomputed; encoder + prefill + decode, one call in flight),
whisper-small, 32 clips, 64 tokens, bf16, EOS masked (min_new_tokens = 64). Three workloads in one process,
interleaved round by round so drift hits them alike; per workload the median of --reps timed rounds after --warmup
rounds (the first two capture the decode graph of each decode context):

  ragged      every clip its own prompt, lengths uniform in 0 .. --max-prompt tokens (wcb_generate_prompted)
  dense_pmax  every clip a prompt as long as the longest of those (its own, extended on the left): the same
              launches over full windows — what padding with real tokens costs (and it changes the transcripts)
  solo        the ragged prompts, one clip per call: 32 calls (the only exact form before)

  python tools/prompt_bench.py [--reps 12] [--warmup 3]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--max-prompt", type=int, default=190)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of fewer calls is not reported)")
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())
    rng = np.random.RandomState(5)
    lens = rng.randint(0, a.max_prompt + 1, a.batch)
    ragged = [rng.randint(300, 20000, n).tolist() for n in lens]
    pmax = int(lens.max())
    dense = [rng.randint(300, 20000, pmax - len(p)).tolist() + p for p in ragged]
    kw = dict(max_length=a.tokens, min_new_tokens=a.tokens)

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "solo":
            ids = torch.cat([m.generate(mel[b:b + 1], prompt_ids=ragged[b] or None, **kw) for b in range(a.batch)])
        else:
            ids = m.generate(mel, prompt_ids=ragged if name == "ragged" else dense, **kw)
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ids

    names = ("ragged", "dense_pmax", "solo")
    times = {k: [] for k in names}
    for k in names:
        for _ in range(max(a.warmup, 2)):
            run(k)
    for _ in range(a.reps):
        for k in names:
            times[k].append(run(k)[0])
    rag_ids, solo_ids = run("ragged")[1], run("solo")[1]
    agree = float((rag_ids == solo_ids).float().mean())   # (bf16: a batch row and a solo row round alike or nearly)
    res = {"model": a.model, "batch": a.batch, "tokens": a.tokens, "dtype": a.dtype, "reps": a.reps,
           "prompt_tokens": {"min": int(lens.min()), "mean": round(float(lens.mean()), 1), "max": pmax},
           "ragged_solo_token_agreement": round(agree, 4)}
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        res[k + "_ms"] = {"median": round(med[k] * 1e3, 3), "min": round(min(v) * 1e3, 3), "max": round(max(v) * 1e3, 3)}
    res["ragged_over_dense_pmax"] = round(med["ragged"] / med["dense_pmax"], 4)
    res["ragged_over_solo"] = round(med["ragged"] / med["solo"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
