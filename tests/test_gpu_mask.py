"""Detection mask of detectAndCompute (cv::SIFT's mask argument; sift_hip_detect_masked*) on the GPU.

Main bar, no tolerance: a masked frame's results equal the SAME configuration's unmasked results with the removed
rows deleted -- kpts3, feats4 and the fp16 descriptor bits, in the same order, in both descriptor modes.  The rows to
delete come from sift_amd.cv.mask_keep (numpy, float32) on the unmasked output; the unmasked path is what the other
test files pin to the oracle.  Small frames are also checked against oracle.detect_and_compute filtered by the same
predicate under the usual bar (keypoints bit-exact, descriptors per parity_bar; the exact mode byte-identical).
"""
import os

import numpy as np
import pytest
from parity_bar import assert_descriptor_bar
from test_gpu_parity import assert_same_keypoints, gpu_keypoints, make_detector, sort_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def snapshot(det):
    """(kpts3, feats4, descriptor bits) of the current frame, copied."""
    det.copyToHost(True)
    return det.final_kpts.copy(), det.final_features.copy(), det.descriptors.view(np.uint16).copy()


def keep_of(ref, mask):
    from sift_amd import cv

    return cv.mask_keep(ref[0][:, 0], ref[0][:, 1], mask)


def filtered(ref, keep):
    return tuple(a[keep] for a in ref)


def assert_same(got, exp, what=""):
    assert len(got[0]) == len(exp[0]), f"{what}: {len(got[0])} keypoints, expected {len(exp[0])}"
    for name, a, b in zip(("kpts3", "feats4", "descriptors"), got, exp):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {name} differ"


def check_filtered_oracle(oracle, cfg, det, img, mask, exact):
    """The current (masked) frame against the oracle's output filtered by the numpy predicate."""
    from sift_amd import cv

    gk, gd, _ = gpu_keypoints(det)
    ok, od = oracle.detect_and_compute(np.asarray(img, np.float32), oracle.from_config(cfg))
    keep = cv.mask_keep(ok["x"], ok["y"], mask)
    ok, od = ok[keep], od[keep]
    assert_same_keypoints(gk, ok)
    gi, oi = sort_keys(gk), sort_keys(ok)
    if exact:
        assert np.array_equal(gd[gi], od[oi])
    else:
        assert_descriptor_bar(gd[gi], od[oi], f"mask {cfg.col_width}x{cfg.row_width} nfeat={cfg.numFeatures}")


def half_plane(w, h, left=True, value=255):
    m = np.zeros((h, w), np.uint8)
    if left:
        m[:, : w // 2] = value
    else:
        m[:, w // 2:] = value
    return m


def checkerboard(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def camera():
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "camera256.npz"))["camera256"][:80, :96])


# ---- 1. identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", [0, 5000])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("upscale", [False, True])
def test_full_mask_is_identity(sift, camera, upscale, exact, nfeat):
    h, w = camera.shape
    assert camera.dtype == np.uint8
    _, det = make_detector(sift, w, h, exact, upscale=upscale, numFeatures=nfeat)
    det.detectAndCompute(camera)
    ref = snapshot(det)
    assert len(ref[0]) >= 10
    for value in (255, 1):
        det.detectAndCompute(camera, np.full((h, w), value, np.uint8))
        assert det.overflow_flags() == 0
        assert_same(snapshot(det), ref, f"all-{value} mask")
    det.detectAndCompute(camera, None)  # mask=None: the unmasked path
    assert_same(snapshot(det), ref, "mask=None")


# ---- 2. empty -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", [0, 50])
def test_zero_mask_is_empty_and_leaves_no_state(sift, nfeat):
    w, h = 256, 256
    img = sift.synth_frame(1, w, h)
    _, fresh = make_detector(sift, w, h, numFeatures=nfeat)
    fresh.detectAndCompute(img)
    ref = snapshot(fresh)
    assert len(ref[0]) > 20
    _, det = make_detector(sift, w, h, numFeatures=nfeat)
    det.detectAndCompute(img, np.zeros((h, w), np.uint8))
    assert det.total_size == 0 and det.overflow_flags() == 0
    det.copyToHost(True)
    assert det.final_kpts.shape == (0, 3) and det.final_features.shape == (0, 4) and det.descriptors.shape == (0, 128)
    k3, f4, ds = det.results_host(True)
    assert k3.shape == (0, 3) and f4.shape == (0, 4) and ds.shape == (0, 128)
    # dedupe bitmap, bucket counts and mask state restored: the next unmasked frame is a fresh handle's
    det.detectAndCompute(img)
    assert_same(snapshot(det), ref, "unmasked frame after an all-zero mask")
    assert det.prev_size == 0


# ---- 3. rounding ----------------------------------------------------------------------------------------------
def test_rounding_is_add_half_then_truncate(sift, oracle):
    w, h = 257, 191
    img = sift.synth_frame(2, w, h)
    mask = checkerboard(w, h)
    cfg, det = make_detector(sift, w, h, upscale=True, numFeatures=0)
    det.detectAndCompute(img)
    ref = snapshot(det)
    keep = keep_of(ref, mask)
    x, y = ref[0][:, 0], ref[0][:, 1]
    trunc = mask[y.astype(np.int32), x.astype(np.int32)] != 0
    assert np.count_nonzero(trunc != keep) > 0, "the input cannot tell (int)(v + 0.5f) from (int)v"
    assert 0 < keep.sum() < len(keep)
    det.detectAndCompute(img, mask)
    assert det.overflow_flags() == 0
    assert_same(snapshot(det), filtered(ref, keep), "checkerboard")
    check_filtered_oracle(oracle, cfg, det, img, mask, False)


# ---- 4. non-255 values and a row stride -----------------------------------------------------------------------
def test_values_and_stride_host_and_device(sift):
    w, h, pad = 256, 256, 37
    img = sift.synth_frame(1, w, h)
    big = np.full((h, w + pad), 255, np.uint8)  # the padding is non-zero: a packed read would keep the wrong points
    big[:, : w // 2] = 0
    big[0::2, w // 2: w] = 1
    big[1::2, w // 2: w] = 7
    view = big[:, :w]
    assert view.strides == (w + pad, 1) and set(np.unique(view)) == {0, 1, 7}
    _, det = make_detector(sift, w, h, numFeatures=0)
    det.detectAndCompute(img)
    ref = snapshot(det)
    keep = keep_of(ref, view)
    assert 0 < keep.sum() < len(keep)
    exp = filtered(ref, keep)
    det.detectAndCompute(img, view)
    assert_same(snapshot(det), exp, "host, strided view")
    dimg, dmask = sift.DeviceArray.from_numpy(img), sift.DeviceArray.from_numpy(big)
    det.detectAndComputeDevice(dimg.value, 4 * w, mask_ptr=dmask.value, mask_stride=w + pad)
    assert_same(snapshot(det), exp, "device, stride")
    det.detectAndComputeDevice(dimg.value, 4 * w)  # no mask: the unmasked call
    assert_same(snapshot(det), ref, "device, unmasked")


# ---- 5. after retainBest --------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_mask_acts_after_retain_best(sift, oracle, exact):
    w, h, n = 256, 256, 50
    img = sift.synth_frame(1, w, h)
    mask = half_plane(w, h)
    cfg, det = make_detector(sift, w, h, exact, numFeatures=n)
    det.detectAndCompute(img)
    ref = snapshot(det)
    keep = keep_of(ref, mask)
    # points on both sides among the unmasked best: "filter first, then keep 50" would answer differently
    assert 0 < keep.sum() < len(keep) and len(keep) >= n
    det.detectAndCompute(img, mask)
    assert det.overflow_flags() == 0
    assert 0 < det.total_size < n
    assert_same(snapshot(det), filtered(ref, keep), "numFeatures=50")
    check_filtered_oracle(oracle, cfg, det, img, mask, exact)


# ---- 6. early rejection (numFeatures = 0) ---------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_early_rejection_keep_all(sift, oracle, exact):
    w, h = 256, 256
    img = sift.synth_frame(1, w, h)
    mask = half_plane(w, h)
    cfg, det = make_detector(sift, w, h, exact, numFeatures=0)
    det.detectAndCompute(img)
    ref = snapshot(det)
    keep = keep_of(ref, mask)
    # keypoints with several orientation peaks (same x, y, size, other angle) on both sides of the edge
    key = np.stack([ref[0][:, 0], ref[0][:, 1], ref[1][:, 1]], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    multi = cnt[inv.reshape(-1)] > 1
    assert np.count_nonzero(multi & keep) >= 2 and np.count_nonzero(multi & ~keep) >= 2
    det.detectAndCompute(img, mask)
    assert det.overflow_flags() == 0
    assert_same(snapshot(det), filtered(ref, keep), "numFeatures=0")
    check_filtered_oracle(oracle, cfg, det, img, mask, exact)
    det.detectAndCompute(img)  # and the handle is as before
    assert_same(snapshot(det), ref, "unmasked frame after a masked one")


# ---- 7. four-kernel order path --------------------------------------------------------------------------------
def test_four_kernel_order_path(sift):
    w, h = 300, 1400  # doubled base, 6 layers: ~33k row buckets > 16384 (test_many_buckets_four_kernel_order)
    img = sift.synth_frame(13, w, h)
    mask = np.zeros((h, w), np.uint8)
    mask[: h // 2] = 255  # the lower half masked out
    _, det = make_detector(sift, w, h, upscale=True, numOctaveLayers=6, numFeatures=700)
    det.detectAndCompute(img)
    ref = snapshot(det)
    keep = keep_of(ref, mask)
    assert 0 < keep.sum() < len(keep)
    det.detectAndCompute(img, mask)
    assert det.overflow_flags() == 0
    assert_same(snapshot(det), filtered(ref, keep), "four-kernel order")
    det.detectAndCompute(img)  # k_bucket_rank re-zeroed the counts of the kept buckets only
    assert_same(snapshot(det), ref, "unmasked frame after a masked one")


# ---- 8. slot[] path of k_order --------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", [0, 60000])  # 60000 > the entries: no threshold, but no early rejection either
def test_order_slot_path(sift, nfeat):
    from test_gpu_paths import blob_field

    w, h = 1280, 960
    img = blob_field(w, h, 50000, 1)
    mask = np.broadcast_to((((np.arange(w) // 16) & 1) * 255).astype(np.uint8), (h, w)).copy()
    _, det = make_detector(sift, w, h, numFeatures=nfeat, maxKeypoints=1 << 16)
    det.detectAndCompute(img)
    assert det.overflow_flags() == 0 and det.total_size > 8192
    ref = snapshot(det)
    keep = keep_of(ref, mask)
    assert 0.3 * len(keep) < keep.sum() < 0.7 * len(keep)
    det.detectAndCompute(img, mask)
    assert det.overflow_flags() == 0
    assert_same(snapshot(det), filtered(ref, keep), "16 px stripes")


# ---- 9. capacity follows the kept count -----------------------------------------------------------------------
def test_capacity_judged_on_kept_count(sift):
    w, h, cap = 752, 480, 257
    img = sift.synth_frame(14, w, h)
    mask = np.zeros((h, w), np.uint8)
    mask[:, : w // 3] = 255
    _, full = make_detector(sift, w, h, numFeatures=0)
    full.detectAndCompute(img)
    ref = snapshot(full)
    keep = keep_of(ref, mask)
    assert len(keep) > cap and 0 < keep.sum() < cap
    _, det = make_detector(sift, w, h, numFeatures=0, maxKeypoints=cap)
    det.detectAndCompute(img)
    assert det.overflow_flags() & 8  # the unmasked frame overflows here (test_max_keypoints_truncates_in_order)
    det.detectAndCompute(img, mask)
    assert det.overflow_flags() == 0
    assert_same(snapshot(det), filtered(ref, keep), "maxKeypoints=257")


# ---- 10. batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", [0, 60])  # 60: retainBest active on every frame (100..128 keypoints)
def test_batch_masks(sift, nfeat):
    w, h, B = 320, 240, 4
    frames = np.stack([sift.synth_frame(30 + i, w, h) for i in range(B)])
    masks = np.stack([np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), half_plane(w, h, left=False),
                      checkerboard(w, h)])
    _, one = make_detector(sift, w, h, numFeatures=nfeat)
    exp = []
    for i in range(B):
        one.detectAndCompute(frames[i], masks[i])
        exp.append(snapshot(one))
    assert len(exp[1][0]) == 0 and 0 < len(exp[2][0]) < len(exp[0][0]) and len(exp[3][0]) > 0
    det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, numFeatures=nfeat), batch=B)
    det.gpuWarmUpAndAllocate()
    dfr, dmk = sift.DeviceArray.from_numpy(frames), sift.DeviceArray.from_numpy(masks)
    det.detectBatchDevice(dfr.value, B, masks_ptr=dmk.value)
    assert det.batch_frames() == B
    for i in range(B):
        n, flags = det.batch_results(i)[:2]
        assert n == len(exp[i][0]) and flags == 0
        k3, f4, d = det.batch_copy_to_host(i)
        assert_same((k3, f4, d.view(np.uint16)), exp[i], f"batch frame {i}")
    # explicit strides, two frames of the four (a partial batch)
    det.detectBatchDevice(dfr.value + 2 * frames[0].nbytes, 2, 4 * w, frames[0].nbytes, masks_ptr=dmk.value + 2 * w * h,
                          mask_stride=w, mask_frame_stride=w * h)
    for i in range(2):
        k3, f4, d = det.batch_copy_to_host(i)
        assert_same((k3, f4, d.view(np.uint16)), exp[2 + i], f"partial batch frame {i}")
    # the single-frame masked call on a batch handle uses frame 0's arena
    det.detectAndCompute(frames[3], masks[3])
    assert_same(snapshot(det), exp[3], "single masked frame on a batch handle")


# ---- 11. frame bookkeeping and matching -----------------------------------------------------------------------
def test_prev_descriptor_and_sidecar_match(sift, oracle):
    w, h = 400, 300
    big = sift.synth_frame(21, w + 8, h + 8)
    a, b = np.ascontiguousarray(big[:h, :w]), np.ascontiguousarray(big[4:4 + h, 6:6 + w])
    mask = half_plane(w, h)
    _, det = make_detector(sift, w, h, numFeatures=0)
    det.detectAndCompute(a)
    ra = snapshot(det)
    det.detectAndCompute(b)
    rb_full = snapshot(det)
    det.detectAndCompute(a)
    det.detectAndCompute(b, mask)
    rb = snapshot(det)
    na, nb = len(ra[0]), len(rb[0])
    assert det.prev_size == na and det.total_size == nb
    assert_same(rb, filtered(rb_full, keep_of(rb_full, mask)), "frame B")
    side = sift.matchBruteForce(det.prev_descriptor, na, det.device_descriptor, nb)
    m = sift.Matcher(na, nb)
    m.set_sidecars(False)
    plain = m.match_host(det.prev_descriptor.data(), na, det.device_descriptor.data(), nb, 0.8, True)
    q, t = ra[2].view(np.float16).astype(np.float32), rb[2].view(np.float16).astype(np.float32)
    oi, _ = oracle.knn2(q, t)
    d2 = np.stack([((q - t[np.maximum(oi[:, k], 0)]) ** 2).sum(axis=1) for k in (0, 1)], 1).astype(np.float32)
    exp = np.where(oi[:, 1] < 0, oi[:, 0], np.where(d2[:, 0] < np.float32(0.8) * d2[:, 1], oi[:, 0], -1))
    assert (exp >= 0).sum() > 20
    assert np.array_equal(side, exp) and np.array_equal(plain, exp)


# ---- 12. errors -----------------------------------------------------------------------------------------------
def test_errors_launch_nothing(sift, tmp_path):
    w, h = 256, 256
    img = sift.synth_frame(1, w, h)
    mask = half_plane(w, h)
    _, det = make_detector(sift, w, h, numFeatures=0)
    det.detectAndCompute(img)
    ref = snapshot(det)
    L, H_ = sift.lib(), det.handle

    def still_current():
        det._refresh()
        assert_same(snapshot(det), ref, "previous results")

    for bad in (np.zeros((h, w + 1), np.uint8), np.zeros((h - 1, w), np.uint8), np.zeros((h, w), np.float32),
                np.zeros((1, h, w), np.uint8)):
        with pytest.raises(sift.SiftHipError):
            det.detectAndCompute(img, bad)
    still_current()
    INVALID, STATE = -1, -3
    dimg, dmask = sift.DeviceArray.from_numpy(img), sift.DeviceArray.from_numpy(mask)
    assert L.sift_hip_detect_masked(H_, img.ctypes.data, 0, sift.SIFT_HIP_F32, mask.ctypes.data, w - 1) == INVALID
    assert b"mask" in L.sift_hip_last_error()
    assert L.sift_hip_detect_device_masked(H_, dimg.value, 0, sift.SIFT_HIP_F32, dmask.value, w - 1, None) == INVALID
    assert L.sift_hip_detect_batch_device_masked(H_, dimg.value, 1, 0, 0, sift.SIFT_HIP_F32, dmask.value, w - 1, 0,
                                                 None) == INVALID
    assert L.sift_hip_detect_masked(H_, img.ctypes.data, 0, 7, mask.ctypes.data, 0) == INVALID
    assert L.sift_hip_detect_device_masked(H_, dimg.value, 0, 7, dmask.value, 0, None) == INVALID
    still_current()
    det.setDataGen(str(tmp_path))
    assert L.sift_hip_detect_masked(H_, img.ctypes.data, 0, sift.SIFT_HIP_F32, mask.ctypes.data, 0) == STATE
    assert L.sift_hip_detect_device_masked(H_, dimg.value, 0, sift.SIFT_HIP_F32, dmask.value, 0, None) == STATE
    with pytest.raises(sift.SiftHipError):
        det.detectAndCompute(img, mask)
    det.setDataGen("")
    assert not os.listdir(tmp_path)
    still_current()
    # NULL mask: the unmasked counterparts
    assert L.sift_hip_detect_masked(H_, img.ctypes.data, 0, sift.SIFT_HIP_F32, None, 0) == 0
    det._refresh()
    assert_same(snapshot(det), ref, "NULL host mask")
    assert L.sift_hip_detect_device_masked(H_, dimg.value, 0, sift.SIFT_HIP_F32, None, 0, None) == 0
    det.sync()
    assert_same(snapshot(det), ref, "NULL device mask")


def test_timing_mode_with_mask(sift):
    w, h = 256, 256
    img = sift.synth_frame(1, w, h)
    mask = half_plane(w, h)
    _, det = make_detector(sift, w, h, numFeatures=0)
    det.detectAndCompute(img, mask)
    ref = snapshot(det)
    det.set_timing(True)
    det.detectAndCompute(img, mask)
    assert_same(snapshot(det), ref, "timing mode")
    assert "orientation" in det.timing()
    det.set_timing(False)
