"""Cost of token-level timestamps (wcb_align): the decode of a fixed-length generate() call and, for the sequences
it produced, the alignment post-pass split by kernel class (per-launch begin/end timestamps of a profiled align()
call: the teacher-forced pass with the capture kernel, the matrix kernel, the DTW kernel), the wall time of the
whole post-pass, and the host alternative on the same matrices: the cross-attention weights' worth of data copied
off the device and transformers' _dynamic_time_warping over the clips on a pool of --threads threads, as a Python
caller would run it in one process (the loop is pure Python: the interpreter lock lets one thread run at a time, so
this is one core's time; a pool of processes could divide it by up to the pool size).

  python tools/align_cost.py [--model small] [--batch 32] [--dtype bf16] [--tokens 64 224] [--reps 7] [--threads 16]
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402


def med_ms(f, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tokens", type=int, nargs="+", default=[64, 224])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    dims = get_dims(a.model)
    m = WhisperCB.from_state_dict(dims, make_weights(dims, seed=0), dtype=a.dtype)
    mel = m.log_mel(torch.from_numpy(synth_batch(a.batch)).cuda())
    enc = m.encode(mel)
    n_heads = (dims.n_layers - dims.n_layers // 2) * dims.n_heads
    try:
        from transformers.models.whisper.generation_whisper import _dynamic_time_warping as hf_dtw
    except ImportError:
        hf_dtw = None
    for n in a.tokens:
        kw = dict(max_length=n, min_new_tokens=n, return_dict_in_generate=True)
        for _ in range(3):   # graphs of both decode contexts, the alignment workspaces
            out = m.generate(mel, return_token_timestamps=True, **kw)
        m.synchronize()
        dec = med_ms(lambda: (m.generate(mel, **kw), m.synchronize()), a.reps)
        both = med_ms(lambda: (m.generate(mel, return_token_timestamps=True, **kw), m.synchronize()), a.reps)
        wall = med_ms(lambda: m.align(enc, out.sequences, 1), a.reps)
        cls = {"pass": [], "capture": [], "matrix": [], "dtw": []}
        for _ in range(a.reps):
            m.profile_enable(True, events=True, stamps=False)
            m.align(enc, out.sequences, 1)
            m.synchronize()
            p = m.profile_read()
            m.profile_enable(False)
            cls["pass"].append(sum(v["ms"] for k, v in p.items() if k.startswith("dec_")))
            cls["capture"].append(p.get("align_capture", {}).get("ms", 0.0))
            cls["matrix"].append(p.get("align_matrix", {}).get("ms", 0.0))
            cls["dtw"].append(p.get("align_dtw", {}).get("ms", 0.0))
        k = {c: statistics.median(v) for c, v in cls.items()}
        line = (f"{a.model} B={a.batch} {a.dtype} {n} tokens, {n_heads} heads: decode {dec:.2f} ms, decode + timestamps "
                f"{both:.2f} ms, align() alone {wall:.2f} ms wall; kernels: teacher-forced pass {k['pass']:.3f} ms + capture "
                f"{k['capture']:.3f} ms, matrix {k['matrix']:.3f} ms, DTW {k['dtw']:.3f} ms")
        if hf_dtw is not None:
            _, mat = m.align(enc, out.sequences, 1, return_matrix=True)
            w_bytes = a.batch * n_heads * (n - 1) * dims.n_audio_ctx * 4
            w_like = torch.empty(w_bytes // 4, dtype=torch.float32, device="cuda")

            def host():
                w_like.cpu()                                   # what HF copies: [B][heads][tokens][1500] f32
                mats = mat.cpu().double().numpy()
                with ThreadPoolExecutor(a.threads) as ex:
                    list(ex.map(lambda b: hf_dtw(mats[b]), range(a.batch)))
            copy = med_ms(lambda: w_like.cpu(), 3)
            host_ms = med_ms(host, 3)
            line += (f"; host alternative: copy of {w_bytes / 2**20:.0f} MiB of weights {copy:.1f} ms, copy + transformers' DTW on "
                     f"{a.threads} threads of one process (one at a time under the interpreter lock) {host_ms:.1f} ms")
        print(line + f" (medians of {a.reps})", flush=True)


if __name__ == "__main__":
    main()
