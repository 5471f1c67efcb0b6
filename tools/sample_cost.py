"""Cost of temperature sampling in the greedy decode: `lm_head` and `dec_select` µs per launch from
profile_read() (HIP events around every launch: the decode runs eagerly and serialised under the profiler),
greedy against sampled on one model — the same build, weights, clips and bias list; passes interleaved.

  python tools/sample_cost.py [--model small] [--batch 32] [--dtype bf16] [--phrases 1000] [--tokens 32] [--reps 3]
"""
import argparse
import os
import sys

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
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())
    phrases = synth_bias_list(a.phrases, eot=dims.eos_token_id) if a.phrases else None
    kw = dict(max_length=a.tokens, min_new_tokens=a.tokens, bias_list=phrases, bias_boost=2.0 if phrases else 0.0)
    modes = {"greedy": {}, "sampled": dict(temperature=1.0, seed=1),
             "greedy+logprobs": dict(output_logprobs=True), "sampled+logprobs": dict(temperature=1.0, seed=1, output_logprobs=True)}
    for extra in modes.values():   # buffers allocated before anything is timed
        m.generate(mel, **kw, **extra)
    m.synchronize()
    rows = {k: [] for k in modes}
    for _ in range(a.reps):
        for name, extra in modes.items():
            m.profile_enable(True, events=True, stamps=False)
            m.generate(mel, **kw, **extra)
            m.synchronize()
            p = m.profile_read()
            m.profile_enable(False)
            rows[name].append({c: (1e3 * p[c]["ms"] / p[c]["launches"], p[c]["launches"], p[c]["kernel"][:60])
                               for c in ("lm_head", "dec_select")})
    print(f"{a.model} B={a.batch} {a.dtype} phrases={a.phrases} tokens={a.tokens}: us per launch, {a.reps} passes", flush=True)
    for name in modes:
        for c in ("lm_head", "dec_select"):
            vals = [r[c][0] for r in rows[name]]
            print(f"  {name:18s} {c:10s} {' '.join(f'{v:7.2f}' for v in vals)}  (launches {rows[name][0][c][1]}, "
                  f"{rows[name][0][c][2]})", flush=True)


if __name__ == "__main__":
    main()
