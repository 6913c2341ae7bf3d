"""bench.py's own options: a plain run times the headline leg and nothing else, ``--full`` adds the other figures, and
``--dump-outputs DIR`` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_full_is_off_by_default_and_implied_by_the_full_record(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full-json", "x.json"])
    assert bench.parse().full


def test_dump_outputs_writes_float32_and_samples_past_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    probs = torch.rand(2, 2, 8, 8, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), {"probs": probs, "loss": torch.tensor(0.5)})
    got = np.load(tmp_path / "a" / "probs.npy")
    assert got.dtype == np.float32 and got.shape == (2, 2, 8, 8) and np.array_equal(got, probs.float().numpy())
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,) and loss[0] == 0.5
    # past the limit: the same seeded sample every time, in proportion to each array's size
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"probs": probs})
    b, c = np.load(tmp_path / "b" / "probs.npy"), np.load(tmp_path / "c" / "probs.npy")
    assert b.dtype == np.float32 and b.shape == (16,) and np.array_equal(b, c)
    assert np.isin(b, probs.float().numpy().ravel()).all()


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_its_outputs(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--size", "128", "--dump-outputs", str(out)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["step_ms"]["n"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "tiles/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert not {"train", "legs", "roofline", "parity", "miou", "cpu_baseline", "full_record"} & set(line)
    probs = np.load(out / "probs.npy")
    assert probs.dtype == np.float32 and probs.shape == (2, 2, 128, 128)
    assert np.allclose(probs.sum(1), 1.0, atol=1e-4)
