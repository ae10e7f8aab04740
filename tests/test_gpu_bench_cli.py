"""bench.py's plain run on the GPU: the headline line only (no side leg unless
--full), --steps timed steps, and --dump-outputs writing the last step's
results -- the rows the single-frame pipeline gives for the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SIDE_LEGS = ("roofline", "cpu_baseline", "exact_descriptors", "host_input", "match_2k", "c4_256_frames_1600x900")


def test_plain_run_and_dump(sift, tmp_path):
    B, steps = 2, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B),
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["unit"] == "Mpix/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["ms_per_step"] > 0 and out["value"] > 0
    # value and ms_per_step describe the same timed steps: B frames of 1920x1200 per step
    # (ms_per_step is printed to 4 decimals, value to 2)
    assert out["value"] == pytest.approx(B * 1920 * 1200 / 1e3 / out["ms_per_step"],
                                         rel=1e-4 / out["ms_per_step"], abs=0.01)
    assert not [k for k in SIDE_LEGS if k in out]

    got = {n[:-4]: np.load(tmp_path / "dump" / n) for n in sorted(os.listdir(tmp_path / "dump"))}
    assert sorted(got) == ["counts", "descriptors", "features", "keypoints"]
    assert got["counts"].dtype == np.float64 and got["counts"].shape == (B,)
    assert all(got[n].dtype == np.float32 for n in ("keypoints", "features", "descriptors"))
    det = sift.Detector(sift.CudaSiftConfig(col_width=1920, row_width=1200, numFeatures=5000, numOctaveLayers=3,
                                            upscale=False, numOctaves=3), device=0)
    det.gpuWarmUpAndAllocate()
    row = 0
    for i in range(B):
        det.detectAndCompute(sift.synth_frame(i, 1920, 1200))
        det.copyToHost(True)
        n = det.total_size
        assert n > 0 and got["counts"][i] == n
        assert np.array_equal(got["keypoints"][row:row + n], det.final_kpts)
        assert np.array_equal(got["features"][row:row + n], det.final_features)
        assert np.array_equal(got["descriptors"][row:row + n], det.descriptors.astype(np.float32))
        row += n
    assert row == len(got["keypoints"]) == len(got["features"]) == len(got["descriptors"])
