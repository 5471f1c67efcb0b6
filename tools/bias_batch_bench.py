"""Per-utterance bias lists against the shared list: whole-call time of generate() (front end excluded:
the mel is precomputed; encoder + decode, one call in flight), whisper-small, 32 clips, 64 tokens, bf16,
EOS masked (min_new_tokens = 64), lambda 2.0. Three workloads in one process, interleaved round by round
so drift hits them alike; per workload the median of --reps timed calls after --warmup calls (the first
two capture the decode graph of each decode context):

  shared      one 1000-phrase list for the whole batch (wcb_generate, the benchmark's boost)
  per_small   1 to 5 phrases per clip, every clip its own (the reference data's shape)
  per_full    every clip the full 1000-phrase list (worst case of the finalize re-score)
  per_full_prebuilt   the same decode through wcb_generate_biased with the forest compiled once, outside the
              timed region (per_full minus the host work of turning 32,000 Python phrase lists into a forest)

  python tools/bias_batch_bench.py [--reps 12] [--warmup 3]

Prints one JSON line.
"""
import argparse
import json
import os
import random
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
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (the median of fewer calls is not reported)")
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())
    full = synth_bias_list(1000, eot=dims.eos_token_id)
    rng = random.Random(11)
    small = [rng.sample(full, rng.randint(1, 5)) for _ in range(a.batch)]
    kw = dict(max_length=a.tokens, min_new_tokens=a.tokens, bias_boost=2.0)
    work = {"shared": dict(bias_list=full), "per_small": dict(bias_lists=small),
            "per_full": dict(bias_lists=[full] * a.batch)}

    import ctypes as C
    from whisper_context_biasing_amd import _lib
    from whisper_context_biasing_amd.model import BiasBatch
    prebuilt = BiasBatch(m, work["per_full"]["bias_lists"])
    work["per_full_prebuilt"] = None

    def generate_prebuilt():
        cfg = _lib.WcbGenCfg(a.tokens, a.tokens, 1, 2.0, 1, 0)
        out = torch.empty(a.batch, a.tokens, dtype=torch.int32, device=m.device)
        steps = C.c_int32(0)
        _lib.check(m._lib.wcb_generate_biased(m._h, mel.data_ptr(), a.batch, C.byref(cfg), prebuilt._h, None, 1,
                                              out.data_ptr(), C.byref(steps),
                                              torch.cuda.current_stream(m.device).cuda_stream), m._h, "wcb_generate_biased")
        return out.to(torch.int64)

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = generate_prebuilt() if name == "per_full_prebuilt" else m.generate(mel, **work[name], **kw)
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ids

    times = {k: [] for k in work}
    for k in work:                       # warm-up: graphs captured, forest buffers at their capacity
        for _ in range(max(a.warmup, 2)):
            run(k)
    for _ in range(a.reps):
        for k in work:
            times[k].append(run(k)[0])
    # the per-utterance decode with one list for all must give the shared decode's ids
    shared_ids = run("shared")[1]
    same = bool(torch.equal(shared_ids, run("per_full")[1]) and torch.equal(shared_ids, run("per_full_prebuilt")[1]))
    res = {"model": a.model, "batch": a.batch, "tokens": a.tokens, "dtype": a.dtype, "reps": a.reps,
           "per_full_equals_shared": same}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(statistics.median(v) * 1e3, 3), "min": round(min(v) * 1e3, 3),
                          "max": round(max(v) * 1e3, 3)}
    # host share of a per-utterance call: compiling the lists into the forest (every call builds its own)
    for k in ("per_small", "per_full"):
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            BiasBatch(m, work[k]["bias_lists"]).close()
            t.append(time.perf_counter() - t0)
        res[k + "_forest_build_ms"] = round(statistics.median(t) * 1e3, 3)
    res["per_small_over_shared"] = round(statistics.median(times["per_small"]) / statistics.median(times["shared"]), 4)
    res["per_full_over_shared"] = round(statistics.median(times["per_full"]) / statistics.median(times["shared"]), 4)
    res["per_full_prebuilt_over_shared"] = round(statistics.median(times["per_full_prebuilt"]) /
                                                 statistics.median(times["shared"]), 4)
    prebuilt.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
