"""Descriptors for caller-supplied keypoints on the GPU (sift_hip_compute*,
Detector.compute / computeDevice) against the detect path and the CPU oracle.

Bars.  The compute chain hands the SAME DescJob list to the SAME descriptor
kernels as detect, so wherever the keypoints are a frame's own, bytes are
identical (no tolerance).  Against oracle.compute_descriptors: the exact mode
is byte-identical for every valid keypoint; the default (fixed-point) mode
keeps its documented |diff| <= 1 for keypoints in the detector's scale range
(size * scale / 2 <= sigma * 2^((L + 0.5) / L)).  Outside that range only the
exact mode and the rows' form are asserted; the default mode's figures are recorded
(parity_bar.record_exact) and quoted in DESIGN.md section 2b.
"""
import os

import numpy as np
import pytest
from parity_bar import DESC_MAX_ABS_DIFF, record_exact

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 3
ANGLES = (0.0, 360.0, 359.99997, 90.0, 17.3, 271.5)
DETECTOR_RANGE = (1.0, 3.2, 6.5)  # size * scale: <= 2 * 1.6 * 2^(3.5 / 3) = 7.18
OVERSIZED_PX = (12.0, 40.0, 200.0)  # size in input pixels; 40 and 200 reach the raster path (radius > 63)


def make(sift, w, h, exact=False, batch=1, **kw):
    cfg = sift.CudaSiftConfig(col_width=w, row_width=h, **kw)
    det = sift.Detector(cfg, exact_descriptors=exact, batch=batch)
    det.gpuWarmUpAndAllocate()
    return cfg, det


def results(sift, det):
    """(keypoint records, kpts3, feats4, descriptor rows as uint16 bits) of the current frame."""
    from sift_amd import cv

    det.copyToHost(True)
    return (cv.keypoint_records(det.final_kpts, det.final_features), det.final_kpts.copy(), det.final_features.copy(),
            det.descriptors.view(np.uint16).copy())


def rows_f32(bits):
    return bits.view(np.float16).astype(np.float32)


def device_rows(sift, ptr, n):
    out = np.empty((n, 128), np.uint16)
    if n:
        sift._check(sift.lib().sift_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "d2h")
    return out


@pytest.fixture(scope="module")
def camera():
    """camera256[:80, :96] (uint8) of the golden file: the 96 x 80 frame of the keypoint grids."""
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "camera256.npz"))["camera256"][:80, :96])


def grid(sift, first, n_oct, w, h, sizes, scaled):
    """Every octave x layer 0..L+2 x six variants: one point at (0, 0) and five uniform in [-2, W+2] x [-2, H+2],
    the angles cycling through ANGLES, the sizes through `sizes` (size * scale when `scaled`, else input pixels)."""
    rng = np.random.default_rng(1)
    out = []
    for o in range(first, first + n_oct):
        for layer in range(L + 3):
            for v in range(6):
                x, y = (0.0, 0.0) if v == 0 else (rng.uniform(-2, w + 2), rng.uniform(-2, h + 2))
                s = sizes[v % len(sizes)]
                out.append((x, y, s * 2.0 ** o if scaled else s, ANGLES[v], 0.01 * (v + 1),
                            (o & 255) | (layer << 8) | ((37 * v) << 16)))
    return np.array(out, sift.KPT_DTYPE)


_oracle_cache = {}


def oracle_rows(oracle, frame, cfg, kpts, key):
    """oracle.compute_descriptors, computed once per (grid, upscale) and shared by the modes."""
    if key not in _oracle_cache:
        od = oracle.compute_descriptors(frame.astype(np.float32), oracle.from_config(cfg), kpts)
        od.flags.writeable = False
        _oracle_cache[key] = od
    return _oracle_cache[key]


# ---- 1. round trip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("w,h,upscale,frame", [(256, 256, False, 1), (257, 191, True, 2)])
def test_round_trip_own_keypoints(sift, oracle, w, h, upscale, frame, exact):
    img = sift.synth_frame(frame, w, h)
    cfg, det = make(sift, w, h, exact, upscale=upscale, numFeatures=0)
    det.detectAndCompute(img)
    kp, k3, f4, desc = results(sift, det)
    assert len(kp) > 20 and det.check_keypoints(kp) == -1
    det.compute(img, kp)
    assert det.total_size == len(kp) and det.overflow_flags() == 0
    kp2, k3b, f4b, desc2 = results(sift, det)
    assert np.array_equal(desc2, desc), f"{np.count_nonzero((desc2 != desc).any(axis=1))} rows differ from detect's"
    assert k3b.tobytes() == k3.tobytes() and f4b.tobytes() == f4.tobytes()
    assert kp2.tobytes() == kp.tobytes()
    if exact:
        assert np.array_equal(rows_f32(desc2), oracle.compute_descriptors(img, oracle.from_config(cfg), kp))


# ---- 2. arbitrary keypoints in the detector's scale range ---------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("upscale", [False, True])
def test_grid_against_oracle(sift, oracle, camera, upscale, exact):
    """Measured on the MI355X.  Exact mode: 0 bytes differ (144 and 216 keypoints).  Default mode: max |diff| 1,
    exact share 0.998481 without and 0.998770 with upscale.  (This test found octave 4 of the upscaled pyramid -- a
    6 x 5 plane -- 2 off on 5 of 4,608 entries while k_descriptor sized its fixed-point scale for the window alone;
    the scale is now also bounded by the plane's interior sample count)"""
    h, w = camera.shape
    cfg, det = make(sift, w, h, exact, upscale=upscale, numFeatures=0)
    first = -1 if upscale else 0
    kp = grid(sift, first, det.nOctaves, w, h, DETECTOR_RANGE, scaled=True)
    assert len(kp) == (216 if upscale else 144) and det.check_keypoints(kp) == -1
    od = oracle_rows(oracle, camera, cfg, kp, ("range", upscale))
    assert np.isfinite(od).all() and od.min() >= 0 and od.max() <= 255
    outside = (kp["x"] < 0) | (kp["y"] < 0) | (kp["x"] > w - 1) | (kp["y"] > h - 1)
    assert outside.sum() >= 10 and (od.max(axis=1) > 0).sum() > len(kp) // 2
    # the 8-bit frame with upscale, the float frame without: both host entry points
    det.compute(camera if upscale else camera.astype(np.float32), kp)
    assert det.total_size == len(kp) and det.overflow_flags() == 0
    kp2, _, _, desc = results(sift, det)
    assert kp2.tobytes() == kp.tobytes()
    gd = rows_f32(desc)
    diff = np.abs(gd - od)
    record_exact(f"compute grid detector-range up={upscale} exact={exact}", diff)
    print(f"up={upscale} exact={exact}: max |diff| {diff.max():.0f}, exact share {(diff == 0).mean():.6f}")
    for o in range(first, first + det.nOctaves):  # per octave: where a miss of the bar sits
        d = diff[((kp["octave"] & 255).astype(np.int8) == o)]
        print(f"  octave {o}: max |diff| {d.max():.0f}, entries > 1: {int((d > 1).sum())}, exact share {(d == 0).mean():.6f}")
    if exact:
        assert np.array_equal(gd, od), f"{np.count_nonzero(diff.max(axis=1))} rows differ, max {diff.max()}"
    else:
        assert diff.max() <= DESC_MAX_ABS_DIFF, f"max |diff| {diff.max()} at keypoint {kp[diff.max(axis=1).argmax()]}"


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("upscale", [False, True])
def test_corners_of_the_validity_box(sift, oracle, camera, upscale, exact):
    """The farthest valid positions (-W, -H) .. (2W, 2H) on the finest and the coarsest octave, small and large:
    windows that miss the plane give all-zero rows, as the oracle's; the rest its bytes (within 1 in the default
    mode, for the sizes of the detector's range).  These are the extremes of the integer window arithmetic.
    The coarsest plane of the upscaled pyramid (6 x 5) holds a one-column window here: the case that needs the
    descriptor's fixed-point scale bounded by the plane's interior."""
    h, w = camera.shape
    cfg, det = make(sift, w, h, exact, upscale=upscale, numFeatures=0)
    first = -1 if upscale else 0
    kp = np.array([(x, y, s * 2.0 ** o, a, 0.02, (o & 255) | (layer << 8))
                   for o, layer in ((first, 0), (first + det.nOctaves - 1, L + 2))
                   for x in (-float(w), 2.0 * w) for y in (-float(h), 2.0 * h)
                   for s, a in ((1.0, 0.0), (6.5, 123.4), (40.0, 360.0))], sift.KPT_DTYPE)
    assert det.check_keypoints(kp) == -1
    od = oracle_rows(oracle, camera, cfg, kp, ("corners", upscale))
    assert (od.max(axis=1) == 0).sum() >= len(kp) // 2
    det.compute(camera, kp)
    assert det.overflow_flags() == 0
    gd = rows_f32(results(sift, det)[3])
    assert not gd[od.max(axis=1) == 0].any()
    if exact:
        assert np.array_equal(gd, od)
    else:  # the +-1 contract covers the detector's scale range: the s = 1.0 and 6.5 keypoints
        in_range = np.tile([True, True, False], len(kp) // 3)
        assert np.abs(gd - od)[in_range].max() <= DESC_MAX_ABS_DIFF


# ---- 3. oversized windows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("upscale", [False, True])
def test_oversized_windows(sift, oracle, camera, upscale, exact):
    """Sizes of 12, 40 and 200 input pixels on every plane: the last two take the descriptor kernels' raster
    path with the radius clamped to the plane diagonal.  Exact mode: the oracle's bytes.  Default mode: rows are
    integers in 0..255; max |diff| and the exact share are recorded, not asserted (measured on the MI355X:
    max |diff| 1 in both pyramids, exact share 0.997613 without upscale and 0.990524 with)."""
    h, w = camera.shape
    cfg, det = make(sift, w, h, exact, upscale=upscale, numFeatures=0)
    kp = grid(sift, -1 if upscale else 0, det.nOctaves, w, h, OVERSIZED_PX, scaled=False)
    assert det.check_keypoints(kp) == -1
    o = (kp["octave"] & 255).astype(np.int32)
    o = np.where(o < 128, o, o - 256)
    radius = np.round(3 * kp["size"] * 2.0 ** -o * 0.5 * np.sqrt(2) * 2.5)
    assert (2 * radius + 1 > 128).sum() > len(kp) // 4, "too few keypoints reach the raster path"
    od = oracle_rows(oracle, camera, cfg, kp, ("oversized", upscale))
    det.compute(camera.astype(np.float32), kp)
    assert det.total_size == len(kp) and det.overflow_flags() == 0
    gd = rows_f32(results(sift, det)[3])
    diff = np.abs(gd - od)
    record_exact(f"compute grid oversized up={upscale} exact={exact}", diff)
    print(f"up={upscale} exact={exact}: max |diff| {diff.max():.0f}, exact share {(diff == 0).mean():.6f}")
    if exact:
        assert np.array_equal(gd, od), f"{np.count_nonzero(diff.max(axis=1))} rows differ, max {diff.max()}"
    else:
        assert gd.min() >= 0 and gd.max() <= 255 and np.array_equal(gd, np.round(gd))


# ---- 4. handle state --------------------------------------------------------------------------------------
def knn(sift, m, qp, nq, tp, nt):
    idx2, d2 = sift.DeviceArray(nq * 8), sift.DeviceArray(nq * 8)
    m.match_device(qp, nq, tp, nt, 0.8, False, idx2.value, d2.value, 0)
    return idx2.to_numpy(np.int32, (nq, 2)), d2.to_numpy(np.float32, (nq, 2))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("computes", [1, 2])
def test_detect_compute_detect_keeps_the_handle_clean(sift, oracle, exact, computes):
    """detect(A) -> compute(B) [-> compute(B)] -> detect(A): the last call's bytes are the first's (the compute
    chain leaves the scratch as the stages it replaces do; one and two computes cross both slot parities), and
    between the calls the frame bookkeeping -- prev_descriptor, counts, sidecars -- is a frame's."""
    w, h = 257, 191
    A, B = sift.synth_frame(4, w, h), sift.synth_frame(5, w, h)
    cfg, det = make(sift, w, h, exact, upscale=True, numFeatures=150)
    det.detectAndCompute(B)
    kpB = results(sift, det)[0]
    det.detectAndCompute(A)
    kpA, k3A, f4A, descA = results(sift, det)
    nA = len(kpA)
    assert nA > 50 and len(kpB) > 50
    m = sift.Matcher(4096, 4096)
    mc = sift.Matcher(4096, 4096)
    mc.set_sidecars(False)
    prev_rows, prev_n = descA, nA
    for c in range(computes):
        kps = kpB if c == 0 else kpB[::-1].copy()
        det.compute(B, kps)
        assert det.total_size == len(kps) and det.prev_size == prev_n and det.overflow_flags() == 0
        q, t = det.prev_descriptor.data(), det.device_descriptor.data()
        assert np.array_equal(device_rows(sift, q, prev_n), prev_rows)
        cur = results(sift, det)[3]
        assert np.array_equal(device_rows(sift, t, len(kps)), cur)
        on = sift.matchBruteForce(det.prev_descriptor, prev_n, det.device_descriptor, len(kps))
        off = mc.match_host(q, prev_n, t, len(kps), 0.8, True)
        assert np.array_equal(on, off)
        gi, gd2 = knn(sift, m, q, prev_n, t, len(kps))
        ci, cd2 = knn(sift, mc, q, prev_n, t, len(kps))
        assert np.array_equal(gi, ci) and np.array_equal(gd2.view(np.uint32), cd2.view(np.uint32))
        oi, odist = oracle.knn2(rows_f32(prev_rows), rows_f32(cur))
        assert np.array_equal(gi, oi)
        assert np.array_equal(np.sqrt(gd2[oi >= 0]).astype(np.float32), odist[oi >= 0])
        prev_rows, prev_n = cur, len(kps)
    det.detectAndCompute(A)
    assert det.overflow_flags() == 0 and det.total_size == nA and det.prev_size == prev_n
    kp3, k3, f4, desc = results(sift, det)
    assert k3.tobytes() == k3A.tobytes() and f4.tobytes() == f4A.tobytes()
    assert np.array_equal(desc, descA)


# ---- 5. device variant ------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_device_variant_flags_bad_keypoints(sift, camera, exact):
    h, w = camera.shape
    cfg, det = make(sift, w, h, exact, upscale=True, numFeatures=0)
    kp = grid(sift, -1, det.nOctaves, w, h, DETECTOR_RANGE, scaled=True)
    bad = kp.copy()
    i0, i1 = 5, len(kp) - 2
    bad["octave"][i0] = (-1 + det.nOctaves) & 255 | (1 << 8)  # one past the last octave
    bad["size"][i1] = np.nan
    assert det.check_keypoints(bad) == i0 and det.check_keypoints(bad[i0 + 1:]) == i1 - i0 - 1
    det.compute(camera, kp)
    host = results(sift, det)[3]
    dimg, dk = sift.DeviceArray.from_numpy(camera), sift.DeviceArray.from_numpy(bad)
    import warnings

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        det.computeDevice(dimg.value, w, dk.value, len(bad), u8=True)
    assert any(issubclass(c.category, sift.SiftKeypointWarning) for c in caught)
    assert det.total_size == len(bad) and det.overflow_flags() == sift.SIFT_HIP_FLAG_BAD_KEYPOINT
    dev = results(sift, det)[3]
    good = np.ones(len(kp), bool)
    good[[i0, i1]] = False
    assert not rows_f32(dev)[~good].any(), "rows of invalid keypoints are not zero"
    assert np.array_equal(dev[good], host[good])
    assert rows_f32(host)[[i0, i1]].any(), "the replaced keypoints had non-zero rows: the zero rows show the check"
    # sidecar of the zero rows: the codes of a zero row (0 - 128) and its key bias
    cp, kpx = det.results_sidecar()
    codes = np.empty((len(bad), 128), np.int8)
    sift._check(sift.lib().sift_hip_memcpy_d2h(codes.ctypes.data, cp, codes.nbytes), "d2h")
    assert np.array_equal(codes.astype(np.int32) + 128, rows_f32(dev).astype(np.int32))
    # n = 0 on both variants: a frame of no keypoints
    det.computeDevice(dimg.value, w, 0, 0, u8=True)
    assert det.total_size == 0 and det.overflow_flags() == 0 and det.prev_size == len(bad)
    det.compute(camera, np.zeros(0, sift.KPT_DTYPE))
    assert det.total_size == 0 and det.prev_size == 0
    # the next detect starts clean
    det.detectAndCompute(camera)
    assert det.overflow_flags() == 0
    n, cur = det.total_size, det.device_descriptor.data()
    # refused lists launch nothing: the detect's results stay current
    cap = det.capacities()["results"]
    with pytest.raises(sift.SiftHipError, match="capacity"):
        det.compute(camera, np.repeat(kp[:1], cap + 1))
    with pytest.raises(sift.SiftHipError, match=f"keypoint {i0} "):
        det.compute(camera, bad)
    with pytest.raises(sift.SiftHipError, match="capacity"):
        det.computeDevice(dimg.value, w, dk.value, cap + 1, u8=True)
    det.sync()
    assert det.total_size == n and det.device_descriptor.data() == cur and det.prev_size == 0


# ---- 6. batch handle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_batch_handle_computes_like_a_single_frame_handle(sift, camera, exact):
    h, w = camera.shape
    rows = []
    for batch in (1, 4):
        cfg, det = make(sift, w, h, exact, batch=batch, upscale=True, numFeatures=0)
        kp = grid(sift, -1, det.nOctaves, w, h, DETECTOR_RANGE, scaled=True)
        det.compute(camera, kp)
        assert det.total_size == len(kp) and det.overflow_flags() == 0
        rows.append(results(sift, det))
    assert np.array_equal(rows[0][3], rows[1][3])
    assert rows[0][1].tobytes() == rows[1][1].tobytes() and rows[0][2].tobytes() == rows[1][2].tobytes()
