"""The descriptor kernels' exact row enumeration (csrc/sift_desc_rows.h) on the GPU.

k_descriptor's enumerated sample loop has no per-sample bin test and no bin clamps: it relies on the rows' exact
intervals.  288 caller-supplied keypoints go through Detector.compute on a 160 x 120 crop of synth_frame(0) and on a
24 x 20 plane: angles on and off the axes, positions on the borders and corners, sizes giving window radius 1, 2, 7,
31, 63 (side 127, the largest enumerated window) and 64 (side 129, the raster path), in both descriptor modes and on
batch-1 and batch-2 handles (k_descriptor<256> and k_descriptor<128>).

* Exact mode: bit-identical to the oracle's compute_descriptors.
* Default mode: byte-identical to tests/golden/desc_rows_default.npy, the rows the library of the commit BEFORE the
  exact enumeration produced for the same keypoints (its sample loop tested every sample of conservative intervals).
  The fixed-point histogram is an exact integer sum, so dropping zero contributions and reordering the rest must not
  move a byte.  Recorded once on an MI355X from a build of that commit:

      tools/ab_build.sh <that commit> parent
      SIFT_HIP_LIB=ab/parent.so python tests/test_gpu_desc_rows.py --record [OUTPUT.npy]

  (the recording also checks that the batch-1 and batch-2 handles of that build agree).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "desc_rows_default.npy")
# size * 5.3033 (= 3 * 0.5 * sqrt(2) * 2.5) rounds to the window radius: 1, 2, 7, 31, 63, 64
SIZES = (0.2, 0.4, 1.32, 5.85, 11.88, 12.07)
RADII = (1, 2, 7, 31, 63, 64)
ANGLES_BIG = (0.0, 90.0, 180.0, 270.0, 45.0, 17.3)
ANGLES_SMALL = (0.0, 270.0, 359.99997, 123.4)


def frames(sift):
    """(160 x 120 crop, 24 x 20 plane) of synth_frame(0)."""
    full = sift.synth_frame(0, 320, 240)
    return np.ascontiguousarray(full[60:180, 80:240]), np.ascontiguousarray(full[50:70, 100:124])


def keypoints(sift, w, h, angles, positions):
    out = []
    for si, s in enumerate(SIZES):
        for ai, a in enumerate(angles):
            for pi, (x, y) in enumerate(positions):
                layer = (si + ai + pi) % 6
                out.append((x, y, s, a, 0.01 * (1 + pi), layer << 8))
    k = np.array(out, sift.KPT_DTYPE)
    radius = np.minimum(np.round(k["size"] * 0.5 * 3 * np.sqrt(2) * 2.5), int(np.hypot(w, h)))
    return k, radius.astype(int)


def cases(sift):
    """[(frame, keypoints, radii)]: the crop with 216 keypoints, the small plane with 72."""
    big, small = frames(sift)
    pos_big = ((0.0, 0.0), (159.0, 119.0), (80.3, 0.4), (0.2, 60.7), (158.6, 61.0), (77.5, 58.2))
    pos_small = ((0.0, 19.0), (23.0, 0.0), (11.6, 9.7))
    out = []
    for img, angles, pos in ((big, ANGLES_BIG, pos_big), (small, ANGLES_SMALL, pos_small)):
        h, w = img.shape
        k, r = keypoints(sift, w, h, angles, pos)
        out.append((img, k, r))
    return out


def compute_rows(sift, img, kp, exact, batch):
    """Descriptor rows (n x 128 uint8) of Detector.compute."""
    h, w = img.shape
    cfg = sift.CudaSiftConfig(col_width=w, row_width=h, upscale=False, numFeatures=0)
    det = sift.Detector(cfg, exact_descriptors=exact, batch=batch)
    det.gpuWarmUpAndAllocate()
    assert det.check_keypoints(kp) == -1
    det.compute(img, kp)
    assert det.total_size == len(kp) and det.overflow_flags() == 0
    det.copyToHost(True)
    rows = det.descriptors.astype(np.float32)
    assert rows.min() >= 0 and rows.max() <= 255 and np.array_equal(rows, np.round(rows))
    return cfg, rows.astype(np.uint8)


def test_cases_cover_the_paths(sift):
    (big, kb, rb), (small, ks, rs) = cases(sift)
    assert big.shape == (120, 160) and small.shape == (20, 24)
    assert len(kb) + len(ks) == 288
    assert sorted(set(rb)) == list(RADII)  # side 127 enumerated, side 129 raster
    assert sorted(set(rs)) == [1, 2, 7, 31]  # clamped to the plane's diagonal
    assert np.load(FIXTURE).shape == (288, 128) and os.path.getsize(FIXTURE) <= 40 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_exact_mode_equals_the_oracle(sift, oracle, batch):
    for img, kp, _ in cases(sift):
        cfg, rows = compute_rows(sift, img, kp, True, batch)
        od = oracle.compute_descriptors(img, oracle.from_config(cfg), kp)
        assert (od.max(axis=1) > 0).sum() > len(kp) // 2
        diff = rows.astype(np.float32) != od
        assert not diff.any(), f"{np.count_nonzero(diff.any(axis=1))} of {len(kp)} rows differ from the oracle's"


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_default_mode_equals_the_recorded_rows(sift, batch):
    want = np.load(FIXTURE)
    at = 0
    for img, kp, _ in cases(sift):
        _, rows = compute_rows(sift, img, kp, False, batch)
        ref = want[at:at + len(kp)]
        at += len(kp)
        bad = (rows != ref).any(axis=1)
        assert not bad.any(), f"{int(bad.sum())} of {len(kp)} rows differ from the recorded ones, first {int(bad.argmax())}"
    assert at == len(want)


def record(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "another-cuda-sift_amd")]
    import sift_amd as sift

    rows = {b: np.concatenate([compute_rows(sift, img, kp, False, b)[1] for img, kp, _ in cases(sift)]) for b in (1, 2)}
    assert np.array_equal(rows[1], rows[2]), "batch-1 and batch-2 handles differ"
    assert (rows[1].max(axis=1) > 0).sum() > len(rows[1]) // 2
    np.save(path, rows[1])
    print(f"{path}: {rows[1].shape} from {sift.LIB_PATH} ({sift.version()})")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
