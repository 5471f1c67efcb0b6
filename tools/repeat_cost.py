"""Cost of the repeat rules in the greedy decode: the same fixed-length generate() call with the rules off and on
(repetition penalty, no-repeat n-gram, both), the kinds interleaved in one script on one model (the same build, the
same weights, one call in flight), the median call time of each and the difference per decode step (as
tools/rules_cost.py measures the token rules). With the rules on, a step pays the per-row bitmap word the LM-head
epilogue reads for every tile and the history pass of the finalize; the call pays one init launch.

  python tools/repeat_cost.py [--model small] [--batch 32] [--dtype bf16] [--tokens 64] [--reps 12]
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
from whisper_context_biasing_amd.synth import synth_batch  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

KINDS = {"off": {}, "penalty": dict(repetition_penalty=1.3), "ngram": dict(no_repeat_ngram_size=3),
         "both": dict(repetition_penalty=1.3, no_repeat_ngram_size=3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())

    def run(kind):
        t0 = time.perf_counter()
        m.generate(mel, max_length=a.tokens, min_new_tokens=a.tokens, **KINDS[kind])   # EOS masked: every call a.tokens steps
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for kind in KINDS:   # each decode context captures the graphs of its kind once (the three ruled kinds share theirs)
        for _ in range(2):
            run(kind)
    ts = {k: [] for k in KINDS}
    for _ in range(a.reps):
        for kind in KINDS:
            ts[kind].append(run(kind))
    med = {k: statistics.median(ts[k]) for k in KINDS}
    print(f"{a.model} B={a.batch} {a.dtype} {a.tokens} tokens: call ms "
          + ", ".join(f"{k} {med[k] * 1e3:.3f}" for k in KINDS) + "; against off, per step: "
          + ", ".join(f"{k} {(med[k] - med['off']) / a.tokens * 1e6:+.2f} us ({100 * (med[k] / med['off'] - 1):+.2f} %)"
                      for k in KINDS if k != "off")
          + f" (medians of {a.reps} interleaved calls)", flush=True)
    for k in KINDS:
        print(f"  {k}, call ms: {[round(t * 1e3, 2) for t in ts[k]]}", flush=True)


if __name__ == "__main__":
    main()
