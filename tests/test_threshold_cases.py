"""What tests/threshold_cases.py's frames do to the detector (no GPU): each
has, by the oracle, the property its GPU test in test_gpu_thresholds.py relies
on.  Capacities are the library's (Detector.capacities(), host-only); the
tile and list sizes mirror another-cuda-sift_amd/csrc/extrema.hip (EX4_LIST,
EX4_COLS and the 2-row / 12-row strips of extrema_block and launch_extrema_all;
EX_LIST, EX_TW x EX_TH of k_extrema) as named constants of threshold_cases.

Candidate counts are those the extrema kernels see: the oracle's set, at a
zero prefilter threshold minus the in-layer-flat candidates
(threshold_cases.library_candidates).  Two findings shape the frames:
  * Period-3 stripes at sigma 1.6 give 16,553 oracle candidates on the spill
    frame, but 15,061 of them are in-layer-flat rounding residue of layers the
    stripes never reach; after the filter its worst 256 x 8 tile holds 322.
    The spill and flood frames therefore use period-4 stripes at sigma 0.6:
    real extrema, every sample of one layer.
  * One full layer of a 256 x 8 tile is exactly EX4_LIST = 2,048 entries
    (2,008 inside the 5-pixel border), so on these frames the 2-row strips
    fill their list to 98 % and no frame here spills the 2-row instantiation
    (a tile holds L layers: hits in non-adjacent layers could exceed 2,048,
    but no generator tried reached it); the spill branch, which the 2-row and
    12-row strips share, runs in the 12-row stream of a batch (10,793 hits in
    the worst tile) and in k_extrema (1,024 against 512).
"""
import numpy as np
import pytest

import threshold_cases as tc


def capacity(sift, w, h, case, **kw):
    det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, **tc.config_kwargs(case, **kw)), device=0)
    return det.capacities()


def candidates(name, img, case, upscale=False):
    return tc.extrema_sets((name, case, upscale), img, tc.oracle_params(case, upscale))


def keypoints(oracle, img, case, upscale=False):
    return oracle.detect_and_compute(img, tc.oracle_params(case, upscale))[0]


def test_prefilter_is_zero_where_stated():
    """thr = 0 for ct / L < 2 / 255: ct <= 0.023 at 3 layers, the default ct from 6 layers."""
    assert [tc.prefilter(c) for c in tc.LAYER_SWEEP] == tc.LAYER_SWEEP_THR
    assert tc.prefilter(tc.ONE_LAYER_REFUSED) == 5
    assert [tc.prefilter(c) for c in tc.CONTRAST_SWEEP] == [0, 0, 1, 4, 12]
    assert all(tc.prefilter(c) == 0 for c in tc.FLAT_CONFIGS + [tc.SPILL6, tc.SPILL7, tc.NOISE])
    assert tc.prefilter((3, 0.023, 10.0, 1.6)) == 0 and tc.prefilter((3, 0.024, 10.0, 1.6)) == 1
    assert tc.prefilter((5, 0.04, 10.0, 1.6)) == 1 and tc.prefilter((6, 0.04, 10.0, 1.6)) == 0
    assert tc.prefilter(tc.FLOOD) == 1  # the flood needs no zero threshold


def test_one_layer_at_default_sigma_is_refused(sift, oracle):
    """(L 1, sigma 1.6) needs 89 taps: the oracle runs it, sift_hip_create refuses it, so the
    sweep's one-layer row runs at sigma 1.0."""
    assert len(keypoints(oracle, tc.blobs(), tc.ONE_LAYER_REFUSED)) > 20
    with pytest.raises(sift.SiftHipError, match="63 taps"):
        capacity(sift, tc.BLOBS_W, tc.BLOBS_H, tc.ONE_LAYER_REFUSED)
    assert capacity(sift, tc.BLOBS_W, tc.BLOBS_H, tc.LAYER_SWEEP[0])["candidates"] > 0


def test_contrast_sweep_moves_the_keypoint_count(oracle):
    n = [len(keypoints(oracle, tc.blobs(), c)) for c in tc.CONTRAST_SWEEP]
    print("contrast sweep keypoints", n)
    assert n[0] >= n[1] > n[2] > n[3] > n[4] == 0, n
    assert n[2] > 100


def test_edge_sweep_moves_the_keypoint_count(oracle):
    """edge 1: (r + 1)^2 / r = 4 and tr^2 < 4 det never holds (AM-GM), so nothing passes; edge 0
    keeps every det > 0 (the test is tr^2 * 0 >= 1 * det), as a huge ratio does."""
    n = {c[2]: len(keypoints(oracle, tc.blobs(), c)) for c in tc.EDGE_SWEEP}
    print("edge sweep keypoints", n)
    assert n[1.0] == 0
    assert 0 < n[1.5] < n[2.0] < n[10.0] < n[100.0] <= n[1e6] == n[0.0]


def test_layer_sweep_has_keypoints(oracle):
    n = [len(keypoints(oracle, tc.blobs(), c)) for c in tc.LAYER_SWEEP]
    print("layer sweep keypoints", n)
    assert min(n) > 100 and len(set(n)) == len(n), n


def test_sweep_has_no_in_layer_flat_candidate():
    """On the blobs frame the filter removes nothing: the sweep compares the plain oracle set."""
    for c in tc.SWEEP:
        full, kept = candidates("blobs", tc.blobs(), c)
        assert len(full) == len(kept) > 100, (c, len(full), len(kept))


def test_noise_is_dense_and_spills_only_the_tall_stream(sift, oracle):
    img = tc.noise(tc.NOISE_W, tc.NOISE_H, 0)
    full, kept = candidates("noise", img, tc.NOISE)
    cap = capacity(sift, tc.NOISE_W, tc.NOISE_H, tc.NOISE, maxKeypoints=32768)
    k = keypoints(oracle, img, tc.NOISE)
    t8, t48 = tc.worst_tile(kept, tc.EX4_COLS, tc.EX4_ROWS_SHORT), tc.worst_tile(kept, tc.EX4_COLS, tc.EX4_ROWS_TALL)
    print(f"noise: {len(kept)} candidates of {cap['candidates']}, {len(k)} keypoints, tiles {t8} / {t48}")
    assert len(full) == len(kept)
    assert tc.ORDER_SLOT_ENTRIES < len(k) <= 32768 == cap["results"]
    assert len(kept) <= 0.6 * cap["candidates"]
    assert t8 < tc.EX4_LIST < t48
    assert not tc.takes_tall_stream(tc.NOISE_W, tc.NOISE_H, 1) and tc.takes_tall_stream(tc.NOISE_W, tc.NOISE_H, 16)


def test_noise_upscaled(sift, oracle):
    img = tc.noise(tc.NOISE_W // 2, tc.NOISE_H // 2, 0)
    full, kept = candidates("noise", img, tc.NOISE, upscale=True)
    cap = capacity(sift, tc.NOISE_W // 2, tc.NOISE_H // 2, tc.NOISE, upscale=True, maxKeypoints=32768)
    k = keypoints(oracle, img, tc.NOISE, upscale=True)
    assert 1000 < len(kept) <= 0.6 * cap["candidates"] and 1000 < len(k) <= cap["results"]


def test_period3_stripes_are_residue_at_default_sigma():
    """The first finding of the header: nothing for a spill test once the flat candidates go."""
    case = (6, 0.04, 10.0, 1.6)
    full, kept = candidates("spill-p3", tc.spill(period=3), case)
    print(f"period-3 spill frame: {len(full)} oracle candidates, {len(kept)} not in-layer-flat")
    assert tc.worst_tile(full, tc.EX4_COLS, tc.EX4_ROWS_SHORT) > tc.EX4_LIST
    assert tc.worst_tile(kept, tc.EX4_COLS, tc.EX4_ROWS_SHORT) < tc.EX4_LIST // 4


def test_spill6(sift, oracle):
    img = tc.spill()
    _, kept = candidates("spill", img, tc.SPILL6)
    cap = capacity(sift, tc.BLOBS_W, tc.BLOBS_H, tc.SPILL6)
    t8, t48 = tc.worst_tile(kept, tc.EX4_COLS, tc.EX4_ROWS_SHORT), tc.worst_tile(kept, tc.EX4_COLS, tc.EX4_ROWS_TALL)
    print(f"spill6: {len(kept)} candidates of {cap['candidates']}, tiles {t8} / {t48}")
    # the 2-row strips' list is filled to the last rows but not overrun (one full layer = EX4_LIST) ...
    assert 0.95 * tc.EX4_LIST < t8 <= tc.EX4_LIST == tc.EX4_COLS * tc.EX4_ROWS_SHORT
    # ... the 12-row stream's overruns several times over; a 16-frame batch takes it
    assert t48 > 4 * tc.EX4_LIST and tc.takes_tall_stream(tc.BLOBS_W, tc.BLOBS_H, 16)
    assert not tc.takes_tall_stream(tc.BLOBS_W, tc.BLOBS_H, 1)
    assert len(kept) <= 0.5 * cap["candidates"]
    assert len(keypoints(oracle, img, tc.SPILL6)) >= 100


def test_spill7(sift, oracle):
    img = tc.spill()
    _, kept = candidates("spill", img, tc.SPILL7)
    cap = capacity(sift, tc.BLOBS_W, tc.BLOBS_H, tc.SPILL7)
    t = tc.worst_tile(kept, tc.EX_TW, tc.EX_TH)
    print(f"spill7: {len(kept)} candidates of {cap['candidates']}, worst 64 x 16 tile {t}")
    assert t > tc.EX_LIST
    assert len(kept) <= 0.5 * cap["candidates"]
    assert len(keypoints(oracle, img, tc.SPILL7)) >= 100


def test_flood(sift, oracle):
    img = tc.flood()
    full, kept = candidates("flood", img, tc.FLOOD)
    cap = capacity(sift, tc.FLOOD_W, tc.FLOOD_H, tc.FLOOD)
    k = keypoints(oracle, img, tc.FLOOD)
    print(f"flood: {len(kept)} candidates ({len(full)} before the filter) of {cap['candidates']}, {len(k)} keypoints")
    assert len(kept) >= 1.15 * cap["candidates"]
    assert 100 <= len(k) <= cap["results"]
    # the frame that follows it on the same handle stays far inside every capacity
    _, after = candidates("follow", tc.flood_follow_up(), tc.FLOOD)
    ka = keypoints(oracle, tc.flood_follow_up(), tc.FLOOD)
    assert len(after) <= 0.1 * cap["candidates"] and 100 <= len(ka) <= cap["results"]


@pytest.mark.parametrize("case", tc.FLAT_CONFIGS, ids=tc.case_id)
def test_sky_floods_only_with_flat_candidates(sift, oracle, case):
    img = tc.sky()
    full, kept = candidates("sky", img, case)
    cap = capacity(sift, tc.BLOBS_W, tc.BLOBS_H, case)["candidates"]
    k = keypoints(oracle, img, case)
    print(f"sky {tc.case_id(case)}: {len(full)} oracle candidates, {len(kept)} not in-layer-flat, capacity {cap}, "
          f"{len(k)} keypoints")
    assert len(full) >= (2 if case[0] == 3 else 1.5) * cap  # 6 layers: 105,598 against 63,975 (1.65 x)
    assert len(kept) <= 0.1 * cap
    assert len(k) >= 100


@pytest.mark.parametrize("case", tc.FLAT_CONFIGS, ids=tc.case_id)
@pytest.mark.parametrize("value", [128, 255])
def test_flat_frames_are_all_residue(oracle, case, value):
    full, kept = candidates(f"flat{value}", tc.flat(value), case)
    print(f"flat {value} {tc.case_id(case)}: {len(full)} oracle candidates")
    assert len(full) > 10000 and len(kept) == 0
    assert len(keypoints(oracle, tc.flat(value), case)) == 0


def test_sky_keypoints_lie_below_the_sky(oracle):
    """The oracle keeps nothing inside the sky (rows 0..129): its keypoints lie below it or on its
    edge.  (That dropping flat candidates changes no result is proved on the GPU, keypoint for
    keypoint against the unfiltered oracle, not here.)"""
    for case in tc.FLAT_CONFIGS:
        k = keypoints(oracle, tc.sky(), case)
        assert k["y"].min() > 100, (case, k["y"].min())
