"""Cost of token rules in the greedy decode: ms per decode step without rules, with deny lists, and with the
timestamp grammar on one model (the same build, the same weights, one call in flight), from the difference of two
fixed-length generate() calls, the three kinds interleaved (as tools/logprob_cost.py measures scoring).

  python tools/rules_cost.py [--model small] [--batch 32] [--dtype bf16] [--phrases 1000] [--reps 7]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

KINDS = {"none": {}, "deny": dict(suppress_tokens=list(range(1, 90)), begin_suppress_tokens=[220]),
         "timestamps": dict(suppress_tokens=list(range(1, 90)), begin_suppress_tokens=[220], return_timestamps=True,
                            max_initial_timestamp=1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=72)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())
    phrases = synth_bias_list(a.phrases, eot=dims.eos_token_id) if a.phrases else None

    def run(n, kind):
        t0 = time.perf_counter()
        m.generate(mel, max_length=n, min_new_tokens=n, bias_list=phrases, bias_boost=2.0 if phrases else 0.0,
                   return_dict_in_generate=True, **KINDS[kind])
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {}
    for n in (a.short, a.long):
        for kind in KINDS:   # each decode context captures the graphs of this length and kind once
            for _ in range(2):
                run(n, kind)
        ts = {k: [] for k in KINDS}
        for _ in range(a.reps):
            for kind in KINDS:   # (a change of kind uploads the bitmaps: part of what a ruled call costs, not of a step)
                ts[kind].append(run(n, kind))
        for kind in KINDS:
            res[(n, kind)] = ts[kind]
    span = a.long - a.short
    per = {k: (statistics.median(res[(a.long, k)]) - statistics.median(res[(a.short, k)])) / span * 1e3 for k in KINDS}
    print(f"{a.model} B={a.batch} {a.dtype} phrases={a.phrases}: decode step "
          + ", ".join(f"{k} {per[k]:.4f} ms" for k in KINDS)
          + f": deny {(per['deny'] - per['none']) * 1e3:+.1f} us / step ({100 * (per['deny'] / per['none'] - 1):+.2f} %), "
          f"timestamps {(per['timestamps'] - per['none']) * 1e3:+.1f} us / step "
          f"({100 * (per['timestamps'] / per['none'] - 1):+.2f} %) (medians of {a.reps} interleaved calls of {a.short} and "
          f"{a.long} tokens)", flush=True)
    for n in (a.short, a.long):
        print(f"  {n} tokens, call ms: " + "; ".join(f"{k} {[round(t * 1e3, 2) for t in res[(n, k)]]}" for k in KINDS), flush=True)


if __name__ == "__main__":
    main()
