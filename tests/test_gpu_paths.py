"""GPU parity on the code paths the default configuration does not take.

* numOctaveLayers > 6: the LDS-staged per-octave extrema kernel (k_extrema)
  instead of the register-streaming all-octave one.
* More than 16384 row buckets (tall, doubled images): retainBest select,
  bucket count, scan and scatter as four kernels instead of k_order.
* More than 8192 oriented entries in k_order (a dense blob field): the
  count/scatter go through slot[] instead of registers.
* maxKeypoints below the keypoint count: results are the first maxKeypoints
  of the full, deterministic output order, and overflow bit 3 is raised.
Same bar as test_gpu_parity.py: keypoints bit-exact, descriptors |diff| <= 1
with >= 99.8 % exact (parity_bar.py).
"""
import numpy as np
import pytest

from test_gpu_parity import assert_same_keypoints, gpu_keypoints, make_detector, sort_keys
from parity_bar import assert_descriptor_bar
from threshold_cases import blob_field, extrema_sets

pytestmark = pytest.mark.gpu


def check_vs_oracle(sift, oracle, cfg, det, img):
    gk, gd, _ = gpu_keypoints(det)
    ok, od = oracle.detect_and_compute(img, oracle.from_config(cfg))
    assert len(ok) > 20
    assert_same_keypoints(gk, ok)
    assert_descriptor_bar(gd[sort_keys(gk)], od[sort_keys(ok)], "paths")


@pytest.mark.parametrize("layers", [7, 9])
def test_many_layers_lds_extrema(sift, oracle, layers):
    w, h = 320, 240
    img = sift.synth_frame(12, w, h)
    cfg, det = make_detector(sift, w, h, upscale=True, numOctaveLayers=layers, numFeatures=0)
    det.detectAndCompute(img)
    cand = det.debug_candidates()
    # thr = floor(0.5 * 0.04 / layers * 255) = 0 here: the oracle also lists the plateaus of
    # rounding residue in the frame's flat parts (2,152 of 3,579 candidates at 7 layers, 18,095 of
    # 19,931 at 9),
    # which the extrema kernels drop (threshold_cases.in_layer_flat).
    full, ref = extrema_sets(("frame12", layers), img, oracle.from_config(cfg))
    assert 1000 < len(ref) < len(full)
    assert np.array_equal(cand[np.lexsort(cand.T[::-1])], ref)
    check_vs_oracle(sift, oracle, cfg, det, img)
    # The exact descriptor mode orders its jobs longest first only up to 8
    # layers; beyond that it takes them in output order: the oracle's bytes
    # either way.
    _, dx = make_detector(sift, w, h, exact_descriptors=True, upscale=True, numOctaveLayers=layers, numFeatures=0)
    dx.detectAndCompute(img)
    assert dx.overflow_flags() == 0
    xk, xd, _ = gpu_keypoints(dx)
    ok, od = oracle.detect_and_compute(img, oracle.from_config(cfg))
    assert_same_keypoints(xk, ok)
    assert np.array_equal(xd[sort_keys(xk)], od[sort_keys(ok)])


def test_many_buckets_four_kernel_order(sift, oracle):
    # doubled 300 x 1400 -> 600 x 2800 base, 6 layers: ~33k row buckets > 16384
    w, h = 300, 1400
    img = sift.synth_frame(13, w, h)
    cfg, det = make_detector(sift, w, h, upscale=True, numOctaveLayers=6, numFeatures=700)
    det.detectAndCompute(img)
    check_vs_oracle(sift, oracle, cfg, det, img)


def test_max_keypoints_truncates_in_order(sift):
    w, h = 752, 480
    img = sift.synth_frame(14, w, h)
    _, full = make_detector(sift, w, h, numFeatures=0)
    full.detectAndCompute(img)
    fk, fd, _ = gpu_keypoints(full)
    assert full.overflow_flags() == 0 and len(fk) > 300
    cap = 257
    _, det = make_detector(sift, w, h, numFeatures=0, maxKeypoints=cap)
    det.detectAndCompute(img)
    assert det.total_size == cap
    assert det.overflow_flags() & 8
    k, d, _ = gpu_keypoints(det)
    assert np.array_equal(k, fk[:cap]) and np.array_equal(d, fd[:cap])


def test_order_many_entries_slot_path(sift, oracle):
    w, h = 1280, 960  # ~5.7k row buckets: k_order, with > 8192 oriented entries
    img = blob_field(w, h, 50000, 1)
    cfg, det = make_detector(sift, w, h, numFeatures=0, maxKeypoints=1 << 16)
    det.detectAndCompute(img)
    assert det.overflow_flags() == 0
    assert det.total_size > 8192, det.total_size
    check_vs_oracle(sift, oracle, cfg, det, img)


def test_device_memory_reference_configs(sift):
    """One Detector at the reference's published configurations (tool default:
    auto octaves, upscale=false, numFeatures=5000) holds at most the device
    memory the reference's readme.md:16 reports (84 / 298 / 214 MiB): the
    per-frame capacities are sized to the frame (sift_hip_capacities)."""
    torch = pytest.importorskip("torch")
    for (w, h, ref_mib) in ((752, 480, 84), (1920, 1200, 298), (1600, 900, 214)):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, numFeatures=5000, upscale=False), device=0)
        det.gpuWarmUpAndAllocate()
        torch.cuda.synchronize()
        used = (free0 - torch.cuda.mem_get_info(0)[0]) / 2**20
        print(f"{w}x{h}: {used:.1f} MiB (reference {ref_mib})")
        assert used <= ref_mib, (w, h, used)
        del det
