"""Cost of token log-probs in the greedy decode: ms per decode step with and without output_logprobs on one
model (the same build, the same weights, one call in flight), from the difference of two fixed-length
generate() calls, scored and unscored repetitions interleaved.

  python tools/logprob_cost.py [--model small] [--batch 32] [--dtype bf16] [--phrases 1000] [--reps 7]
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

    def run(n, scored):
        t0 = time.perf_counter()
        out = m.generate(mel, max_length=n, min_new_tokens=n, bias_list=phrases, bias_boost=2.0 if phrases else 0.0,
                         output_logprobs=scored, return_dict_in_generate=True)
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    res = {}
    for n in (a.short, a.long):
        for scored in (False, True):   # each decode context captures both graphs of this length once
            for _ in range(2):
                _, out = run(n, scored)
            res[("ids", n, scored)] = out.sequences
        ts = {False: [], True: []}
        for _ in range(a.reps):
            for scored in (False, True):
                ts[scored].append(run(n, scored)[0])
        for scored in (False, True):
            res[(n, scored)] = ts[scored]
        assert torch.equal(res[("ids", n, False)], res[("ids", n, True)]), "scoring changed an id"
    span = a.long - a.short
    per = {s: (statistics.median(res[(a.long, s)]) - statistics.median(res[(a.short, s)])) / span * 1e3 for s in (False, True)}
    lo = {s: (min(res[(a.long, s)]) - min(res[(a.short, s)])) / span * 1e3 for s in (False, True)}
    print(f"{a.model} B={a.batch} {a.dtype} phrases={a.phrases}: decode step unscored {per[False]:.4f} ms "
          f"(min-based {lo[False]:.4f}), scored {per[True]:.4f} ms (min-based {lo[True]:.4f}): "
          f"{(per[True] - per[False]) * 1e3:+.1f} us / step, {100 * (per[True] / per[False] - 1):+.2f} % "
          f"(medians of {a.reps} interleaved calls of {a.short} and {a.long} tokens)", flush=True)
    for n in (a.short, a.long):
        print(f"  {n} tokens, call ms: unscored {[round(t * 1e3, 2) for t in res[(n, False)]]} "
              f"scored {[round(t * 1e3, 2) for t in res[(n, True)]]}", flush=True)


if __name__ == "__main__":
    main()
