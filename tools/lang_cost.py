"""Cost of language detection in the greedy decode: wall ms of generate(language="auto") against the same call with
every clip's language given (the detected ids), on one model — the same build, the same weights, one call in flight,
the two kinds of call interleaved. "auto" adds one decoder pass over [start], the language head and its finalize
between the encoder and the prefill; the decode steps replay the same graphs.

  python tools/lang_cost.py [--model small] [--batch 32] [--dtype bf16] [--tokens 64] [--reps 7]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit("--reps: medians of at least 7 calls")
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())
    n = a.tokens

    def run(language):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(mel, language=language, max_length=n, min_new_tokens=n, return_dict_in_generate=True)
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    detected = run("auto")[1].languages.tolist()
    route = "per-clip" if len(set(detected)) > 1 else "flat"   # (a list of equal languages takes the flat prefix)
    for _ in range(2):            # each decode context captures its graphs once
        for language in ("auto", detected):
            ids = run(language)[1].sequences
    ts = {"auto": [], "given": []}
    for _ in range(a.reps):
        t, out = run("auto")
        ts["auto"].append(t)
        assert torch.equal(out.sequences, ids), "auto changed an id"
        t, out = run(detected)
        ts["given"].append(t)
        assert torch.equal(out.sequences, ids), "the given languages changed an id"
    med = {k: statistics.median(v) * 1e3 for k, v in ts.items()}
    print(f"{a.model} B={a.batch} {a.dtype} {n} tokens: generate(language=\"auto\") {med['auto']:.3f} ms, languages given "
          f"{med['given']:.3f} ms: {med['auto'] - med['given']:+.3f} ms / call, {100 * (med['auto'] / med['given'] - 1):+.2f} % "
          f"(medians of {a.reps} interleaved calls; min {min(ts['auto']) * 1e3:.3f} / {min(ts['given']) * 1e3:.3f} ms)", flush=True)
    for k in ("auto", "given"):
        print(f"  {k}: call ms {[round(t * 1e3, 2) for t in ts[k]]}", flush=True)
    print(f"  graph_captures {m.debug_counter('graph_captures')}, distinct detected languages {len(set(detected))} "
          f"(the given call takes the {route} route)", flush=True)


if __name__ == "__main__":
    main()
