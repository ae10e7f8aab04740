"""GPU parity of the Gaussian pyramid at every blur radius and staging path.

tests/blur_cases.py lists configurations whose layer blurs take every radius
1..31 (tests/test_blur_cases.py proves it); each runs on a 201 x 197 frame:
4 x 4 ragged blur tiles with an interior 16-byte-staged tile for every
radius, interior-row tiles, all four border kinds, and octaves down to 6 x 6
that go through the pyramid tail (radii <= 16) or through k_blur with planes
narrower than the radius (multi-bounce reflection).  The bar is the suite's:
Gaussian planes, candidates and keypoints bit-exact against the oracle,
descriptors within 1 -- the exact fraction is printed, not asserted: these
radii give window sizes the 99.8 % bar was never measured at.

Also: frames that straddle the border staging's one-reflection shortcut,
float frames with negative pixels (the tail's zero-padded taps), and the
four-wave blur kernels at radii the default pyramid never launches them with.
"""
import numpy as np
import pytest

import blur_cases as bc
from parity_bar import record_exact
from threshold_cases import library_candidates
from test_gpu_parity import assert_same_keypoints, gpu_keypoints, make_detector, sort_keys

pytestmark = pytest.mark.gpu


def assert_planes(det, pyr, tag):
    assert det.nOctaves == len(pyr), tag
    for o, planes in enumerate(pyr):
        for layer in range(planes.shape[0]):
            g = det.debug_gaussian(o, layer)
            assert g.shape == planes[layer].shape
            bad = np.count_nonzero(g.view(np.uint32) != planes[layer].view(np.uint32))
            assert bad == 0, (f"{tag} octave {o} ({g.shape[1]} x {g.shape[0]}) layer {layer}: {bad} pixels differ "
                              f"(max |d| {np.abs(g - planes[layer]).max()})")


def assert_keypoints_and_descriptors(det, ok, od, tag):
    """Keypoints bit-exact, no overflow, descriptors |gpu - oracle| <= 1; returns the exact fraction."""
    assert det.overflow_flags() == 0, tag
    gk, gd, _ = gpu_keypoints(det)
    assert_same_keypoints(gk, ok)
    diff = np.abs(gd[sort_keys(gk)] - od[sort_keys(ok)])
    record_exact(f"blur sweep {tag}", diff)
    exact = float((diff == 0).mean()) if diff.size else 1.0
    print(f"blur sweep {tag}: {len(ok)} keypoints, descriptor exact fraction {exact:.6f} "
          f"({int((diff != 0).sum())} of {diff.size} entries differ)")
    assert diff.size == 0 or diff.max() <= 1, f"{tag} descriptor max |diff| {diff.max()}"
    return exact


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_sweep_vs_oracle(sift, oracle, case):
    """Measured descriptor exact fractions (MI355X): 0.9997-0.9999 for sigma <=
    0.6 (437-904 keypoints), 0.9990-0.9995 for sigma 1.0-1.6, 0.9944-0.9965 for
    2.35-3.65, 0.9818-0.9900 for 4.3-5.0 (9-26 keypoints, the widest windows)."""
    img = bc.sweep_frame(sift)
    init, layers = bc.radii(case)
    tag = f"{bc.case_id(case)} radii {init} {layers}"
    cfg, det = make_detector(sift, bc.SWEEP_W, bc.SWEEP_H, **bc.config_kwargs(case))
    det.detectAndCompute(img)
    p = oracle.from_config(cfg)
    assert_planes(det, oracle.gaussian_pyramid(img, p), tag)
    cand, ref = det.debug_candidates(), oracle.extrema(img, p)
    ref = library_candidates(img, p, ref)  # thr = 0 (6, 9 layers): without the in-layer-flat plateaus (389 at s0.6-L9)
    assert cand.shape == ref.shape, f"{tag}: candidates gpu={len(cand)} oracle={len(ref)}"
    assert np.array_equal(cand[np.lexsort(cand.T[::-1])], ref[np.lexsort(ref.T[::-1])]), tag
    ok, od = bc.oracle_keypoints(sift, case)
    assert_keypoints_and_descriptors(det, ok, od, tag)


@pytest.mark.parametrize("case", bc.ONE_BOUNCE_CASES, ids=bc.case_id)
def test_one_bounce_switch(sift, oracle, case):
    """The border staging reflects once when W > R + 1 && H > R + 1 and loops
    otherwise, per plane's own radius: frames of one octave whose sides sit on
    both sides of that for the smallest and the largest radius, planes only."""
    for w, h in bc.one_bounce_sizes(case):
        img = sift.synth_frame(40, w, h)
        cfg, det = make_detector(sift, w, h, **bc.config_kwargs(case, numOctaves=1))
        det.detectAndCompute(img)
        assert_planes(det, oracle.gaussian_pyramid(img, oracle.from_config(cfg)), f"{bc.case_id(case)} {w} x {h}")


@pytest.mark.parametrize("case", [(1.6, 3, False), bc.NEGATIVE_CASE], ids=bc.case_id)
def test_negative_pixels(sift, oracle, case):
    """A float frame of about -128..127.  The tail pads every plane's taps
    with zeros to its radius class, which is bit-exact only while a zero
    weight adds a signed zero to the running sum: that must hold for negative
    sums too, as must the descriptor's pixel range."""
    img = bc.sweep_frame(sift, -128.0)
    assert img.min() < -100 and img.max() > 100
    tag = f"{bc.case_id(case)} frame - 128"
    cfg, det = make_detector(sift, bc.SWEEP_W, bc.SWEEP_H, **bc.config_kwargs(case))
    assert bc.tail_class(bc.radii(case)[1]) is not None
    det.detectAndCompute(img)
    assert_planes(det, oracle.gaussian_pyramid(img, oracle.from_config(cfg)), tag)
    ok, od = bc.oracle_keypoints(sift, case, -128.0)
    assert len(ok) > 20, "fixture too small to be meaningful"
    assert_keypoints_and_descriptors(det, ok, od, tag)


def test_four_wave_blur_other_radii(sift):
    """blur_waves picks the four-wave kernels from 2048 tiles per launch: 64
    frames of 512 x 256 (32 tiles each) in one batch, one octave, at radii
    6..14.  Frames 0, 31 and 63 equal the same frames through a single-frame
    detector (eight-wave kernels), which the sweep holds to the oracle."""
    w, h, n = 512, 256, 64
    case = bc.FOUR_WAVE_CASE
    frames = np.stack([sift.synth_frame(100 + i, w, h) for i in range(n)])
    assert (w // 64) * (h // 64) * n >= 2048
    dev = sift.DeviceArray.from_numpy(frames)
    cfg = sift.CudaSiftConfig(col_width=w, row_width=h, **bc.config_kwargs(case, numOctaves=1))
    batch = sift.Detector(cfg, device=0, batch=n)
    batch.gpuWarmUpAndAllocate()
    batch.detectBatchDevice(dev.value, n, w * 4, h * w * 4, sync=True)
    assert batch.batch_frames() == n
    _, one = make_detector(sift, w, h, **bc.config_kwargs(case, numOctaves=1))
    for i in (0, 31, 63):
        one.detectAndCompute(frames[i])
        one.copyToHost(True)
        count, flags = batch.batch_results(i)[:2]
        k3, f4, d = batch.batch_copy_to_host(i)
        assert flags == 0 and one.overflow_flags() == 0
        assert count == one.total_size > 20, (i, count, one.total_size)
        assert np.array_equal(k3.view(np.uint32), one.final_kpts.view(np.uint32)), i
        assert np.array_equal(f4.view(np.uint32), one.final_features.view(np.uint32)), i
        assert np.array_equal(d.view(np.uint16), one.descriptors.view(np.uint16)), i
