"""bench.py's plain run and `--dump-outputs`: the arrays of the last timed step as float32 .npy files
(a fixed sample when over the byte budget), and a plain run's line without what `--full` adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_and_samples_over_budget(tmp_path):
    ids = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"ids": ids, "big": big}, max_bytes=2 * 4 * 100)
    a_ids, a_big = np.load(tmp_path / "a" / "ids.npy"), np.load(tmp_path / "a" / "big.npy")
    assert a_ids.dtype == a_big.dtype == np.float32
    np.testing.assert_array_equal(a_ids, ids.numpy())                    # under its share: whole, own shape
    assert a_big.shape == (100,) and np.all(np.diff(a_big) > 0)          # a sample of distinct elements, in order
    assert a_ids.nbytes + a_big.nbytes <= 2 * 4 * 100
    bench.dump_outputs(str(tmp_path / "b"), {"big": big + 0.0, "ids": ids}, max_bytes=2 * 4 * 100)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "big.npy"), a_big)   # the same elements every time


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 2 and "--steps must be >= 1" in p.stderr


@pytest.mark.gpu
def test_plain_run_dumps_last_step_and_leaves_full_parts_out(tmp_path):
    """One plain run at a small shape (tiny.en, 3 clips, 8 tokens): the line's contract fields, nothing of
    `--full`, token ids in the dumped `ids`, and the dumped `mel` equal to the package's log-mel of the
    same seeded clips."""
    steps, B, T = 2, 3, 8
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--model", "tiny.en", "--batch", str(B), "--new-tokens", str(T),
                        "--bias-phrases", "50", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [s for s in p.stdout.splitlines() if s.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "audio-seconds/sec" and out["dtype"] == "bf16"
    assert abs(out["value"] - B * 30.0 / (out["ms_per_step"] * 1e-3)) <= 0.01 * out["value"]
    assert out["cpu_baseline"] is None and out["biased_wer"] is None and not out["phases"]
    assert set(out["roofline"]) == {"step"}
    ids, mel = np.load(tmp_path / "out" / "ids.npy"), np.load(tmp_path / "out" / "mel.npy")
    assert sorted(os.listdir(tmp_path / "out")) == ["ids.npy", "mel.npy"]
    assert ids.dtype == mel.dtype == np.float32 and ids.shape == (B, T) and mel.shape[0] == B

    from whisper_context_biasing_amd.config import get_dims
    from whisper_context_biasing_amd.model import WhisperCB
    from whisper_context_biasing_amd.shard import broadcast_weights
    from whisper_context_biasing_amd.synth import synth_batch
    dims = get_dims("tiny.en")
    assert np.array_equal(ids, np.round(ids)) and ids.min() >= 0 and ids.max() < dims.vocab
    dev = torch.device("cuda", 0)
    model = WhisperCB.from_state_dict(dims, broadcast_weights(dims, dev, seed=0, views=True), dtype="bf16", device=0)
    ref_mel = model.log_mel(torch.from_numpy(synth_batch(B)).to(dev)).float().cpu().numpy()
    np.testing.assert_array_equal(mel, ref_mel)
