"""GPU parity away from contrastThreshould 0.04 / edgeThreshould 10, and on
candidate lists that are dense, that overrun a workgroup's LDS list, that
overrun the frame's list, or that flat regions would flood.

tests/threshold_cases.py holds the frames and configurations,
tests/test_threshold_cases.py proves on the CPU what each one reaches.  The
bar is the suite's: candidates equal the oracle's set (minus the
in-layer-flat ones, which the extrema kernels drop), keypoints bit-exact on
all six fields, descriptors within 1 per byte, byte-identical in the exact
mode.  The exact share of the default mode is printed per case; measured on
an MI355X it is 0.99893 or more on every case here (sweep 0.99917-0.99976,
noise 0.99997, spill 0.99983-0.99984, sky 0.99893-0.99947, the subsets that
survive the candidate overflow 0.99987-0.99990), so parity_bar's 99.8 % is
asserted throughout.
"""
import numpy as np
import pytest

import threshold_cases as tc
from parity_bar import DESC_EXACT_MIN, record_exact
from test_gpu_parity import assert_same_keypoints, gpu_keypoints, make_detector, sort_keys

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave")


def run(sift, img, case, **kw):
    h, w = img.shape
    cfg, det = make_detector(sift, w, h, **tc.config_kwargs(case, **kw))
    det.detectAndCompute(img)
    return cfg, det


def assert_candidates(det, kept, tag):
    cand, hits = det.debug_candidates(return_count=True)
    assert hits == len(cand) == len(kept), f"{tag}: candidates gpu={hits} (stored {len(cand)}) oracle={len(kept)}"
    assert np.array_equal(tc.sort_rows(cand), kept), tag


def assert_descriptors(gd, od, tag):
    """parity_bar's bar: |gpu - oracle| <= 1 on every byte and >= 99.8 % of them equal; the share is printed."""
    diff = np.abs(gd - od)
    record_exact(f"thresholds {tag}", diff)
    exact = float((diff == 0).mean()) if diff.size else 1.0
    print(f"thresholds {tag}: {len(gd)} keypoints, descriptor exact share {exact:.6f} "
          f"({int((diff != 0).sum())} of {diff.size} entries differ)")
    assert diff.size == 0 or diff.max() <= 1, f"{tag} descriptor max |diff| {diff.max()}"
    assert exact >= DESC_EXACT_MIN, f"{tag} exact share {exact:.6f} < {DESC_EXACT_MIN}"
    return exact


def assert_results(det, ok, od, tag, exact_mode=False):
    """No overflow, keypoints bit-exact as a set, descriptors at the bar of the handle's mode."""
    assert det.overflow_flags() == 0, tag
    if len(ok) == 0:
        assert det.total_size == 0, tag
        return
    gk, gd, _ = gpu_keypoints(det)
    assert_same_keypoints(gk, ok)
    gd, od = gd[sort_keys(gk)], od[sort_keys(ok)]
    if exact_mode:
        assert np.array_equal(gd, od), f"{tag}: {np.count_nonzero((gd != od).any(1))} exact-mode descriptors differ"
    else:
        assert_descriptors(gd, od, tag)


def check_both_modes(sift, name, img, case, tag, upscale=False, **kw):
    """Candidates, keypoints and descriptors of one frame against the oracle, default and exact mode."""
    p = tc.oracle_params(case, upscale)
    ok, od = tc.oracle_keypoints((name, case, upscale), img, p)
    _, det = run(sift, img, case, upscale=upscale, **kw)
    assert_candidates(det, tc.extrema_sets((name, case, upscale), img, p)[1], tag)
    assert_results(det, ok, od, tag)
    _, dx = run(sift, img, case, upscale=upscale, exact_descriptors=True, **kw)
    assert_results(dx, ok, od, tag + " exact", exact_mode=True)
    return det


# --- 1. threshold sweep -----------------------------------------------------------
@pytest.mark.parametrize("case", tc.SWEEP, ids=tc.case_id)
def test_threshold_sweep(sift, oracle, case):
    """Measured exact shares (MI355X): 0.999168-0.999756 over the 13 rows with keypoints (154-624)."""
    img = tc.blobs()
    check_both_modes(sift, "blobs", img, case, f"blobs {tc.case_id(case)}")
    if case in (tc.CONTRAST_SWEEP[-1], tc.EDGE_SWEEP[1]):
        assert len(tc.oracle_keypoints(("blobs", case, False), img, tc.oracle_params(case))[0]) == 0


# --- 2. dense frames ----------------------------------------------------------------
def test_noise_single_frame(sift, oracle):
    """14,591 candidates, 19,091 keypoints: more than 8,192 oriented entries.  Measured exact share
    0.999976 (upscaled: 0.999966)."""
    img = tc.noise(tc.NOISE_W, tc.NOISE_H, 0)
    det = check_both_modes(sift, "noise0", img, tc.NOISE, "noise", maxKeypoints=32768)
    assert det.total_size > tc.ORDER_SLOT_ENTRIES


def test_noise_upscaled(sift, oracle):
    img = tc.noise(tc.NOISE_W // 2, tc.NOISE_H // 2, 0)
    check_both_modes(sift, "noise0", img, tc.NOISE, "noise upscaled", upscale=True, maxKeypoints=32768)


def batch_detect(sift, frames, case, **kw):
    n, h, w = frames.shape
    cfg = sift.CudaSiftConfig(col_width=w, row_width=h, **tc.config_kwargs(case, **kw))
    det = sift.Detector(cfg, device=0, batch=n)
    det.gpuWarmUpAndAllocate()
    dev = sift.DeviceArray.from_numpy(frames)
    det.detectBatchDevice(dev.value, n, w * 4, h * w * 4, sync=True)
    assert det.batch_frames() == n
    return det, dev


def batch_keypoints(det, i):
    """Frame i of a batch as gpu_keypoints gives a single frame."""
    k, f, d = det.batch_copy_to_host(i)
    out = np.zeros(len(k), tc.oracle.KPT_DTYPE)
    out["x"], out["y"], out["size"] = k[:, 0], k[:, 1], f[:, 1]
    out["angle"], out["response"], out["octave"] = f[:, 3], f[:, 2], f[:, 0].astype(np.int64).astype(np.int32)
    return out, d.astype(np.float32)


def assert_batch_equals_single(det, one, frames, tag):
    """Every frame of the batch bit-equal, in order, to the same frame through the single-frame handle."""
    for i, img in enumerate(frames):
        one.detectAndCompute(img)
        one.copyToHost(True)
        count, flags = det.batch_results(i)[:2]
        k3, f4, d = det.batch_copy_to_host(i)
        assert flags == 0 and one.overflow_flags() == 0, (tag, i, flags)
        assert count == one.total_size > 100, (tag, i, count, one.total_size)
        assert np.array_equal(k3.view(np.uint32), one.final_kpts.view(np.uint32)), (tag, i)
        assert np.array_equal(f4.view(np.uint32), one.final_features.view(np.uint32)), (tag, i)
        assert np.array_equal(d.view(np.uint16), one.descriptors.view(np.uint16)), (tag, i)


def test_noise_batch_takes_the_tall_stream(sift, oracle):
    """16 noise frames in one launch: octave 0 streams 12 rows per wave, and its worst 256 x 48
    tile (2,518 hits on seed 0) overruns the LDS list into the frame's list."""
    n = 16
    frames = np.stack([tc.noise(tc.NOISE_W, tc.NOISE_H, s) for s in range(n)])
    assert tc.takes_tall_stream(tc.NOISE_W, tc.NOISE_H, n)
    det, _dev = batch_detect(sift, frames, tc.NOISE, maxKeypoints=32768)
    _, one = make_detector(sift, tc.NOISE_W, tc.NOISE_H, **tc.config_kwargs(tc.NOISE, maxKeypoints=32768))
    assert_batch_equals_single(det, one, frames, "noise batch")
    for i in (0, n - 1):
        ok, od = tc.oracle_keypoints((f"noise{i}", tc.NOISE, False), frames[i], tc.oracle_params(tc.NOISE))
        gk, gd = batch_keypoints(det, i)
        assert_same_keypoints(gk, ok)
        assert_descriptors(gd[sort_keys(gk)], od[sort_keys(ok)], f"noise batch frame {i}")


# --- 3. LDS-list spill ----------------------------------------------------------------
@pytest.mark.parametrize("case", [tc.SPILL6, tc.SPILL7], ids=tc.case_id)
def test_spill_single_frame(sift, oracle, case):
    """Period-4 stripes: every sample of one layer is an extremum.  7 layers: k_extrema's 64 x 16
    tiles hold 1,024 hits against a list of 512.  6 layers: the 2-row strips' worst tile holds
    2,008 of 2,048 (one full layer of a 256 x 8 tile is the list's size), so no frame here spills
    the 2-row instantiation; test_spill6_batch runs the branch it shares with the 12-row stream.
    Twice on one handle: the same results, whatever order the atomics took."""
    img = tc.spill()
    tag = f"spill {tc.case_id(case)}"
    det = check_both_modes(sift, "spill", img, case, tag)
    first = (det.debug_candidates(), *gpu_keypoints(det))
    det.detectAndCompute(img)
    again = (det.debug_candidates(), *gpu_keypoints(det))
    assert det.overflow_flags() == 0
    assert np.array_equal(tc.sort_rows(first[0]), tc.sort_rows(again[0]))
    for a, b in zip(first[1:], again[1:]):
        assert np.array_equal(a, b), tag


def test_spill6_batch(sift, oracle):
    """The spill frame 16 times in one launch: the 12-row stream's worst 256 x 48 tile holds 10,793
    hits, so four fifths of them take the spill branch (the one the 2-row strips share)."""
    n = 16
    frames = np.stack([tc.spill()] * n)
    assert tc.takes_tall_stream(tc.BLOBS_W, tc.BLOBS_H, n)
    det, _dev = batch_detect(sift, frames, tc.SPILL6)
    _, one = make_detector(sift, tc.BLOBS_W, tc.BLOBS_H, **tc.config_kwargs(tc.SPILL6))
    one.detectAndCompute(frames[0])
    one.copyToHost(True)
    ok, od = tc.oracle_keypoints(("spill", tc.SPILL6, False), frames[0], tc.oracle_params(tc.SPILL6))
    for i in range(n):
        count, flags = det.batch_results(i)[:2]
        k3, f4, d = det.batch_copy_to_host(i)
        assert flags == 0 and count == one.total_size == len(ok), (i, flags, count)
        assert np.array_equal(k3.view(np.uint32), one.final_kpts.view(np.uint32)), i
        assert np.array_equal(f4.view(np.uint32), one.final_features.view(np.uint32)), i
        assert np.array_equal(d.view(np.uint16), one.descriptors.view(np.uint16)), i
    gk, gd = batch_keypoints(det, n - 1)
    assert_same_keypoints(gk, ok)
    assert_descriptors(gd[sort_keys(gk)], od[sort_keys(ok)], "spill batch frame 15")


# --- 4. overflow of the frame's candidate list ----------------------------------------------
def rows_as_keys(k):
    """Keypoints as one opaque key per row (all six fields, bit for bit)."""
    a = np.zeros((len(k), 6), np.uint32)
    for j, f in enumerate(FIELDS):
        a[:, j] = k[f].view(np.uint32)
    return [r.tobytes() for r in a]


def assert_overflowed_subset(gk, gd, flags, ok, od, tag):
    """What must hold for any subset of the candidates: flag 1 alone, and the keypoints a
    duplicate-free subset of the oracle's, bit-exact per field, descriptors at the bar against their rows'."""
    assert flags == 1, (tag, flags)
    index = {key: i for i, key in enumerate(rows_as_keys(ok))}
    assert len(index) == len(ok), "oracle keypoints are not distinct"
    keys = rows_as_keys(gk)
    assert len(set(keys)) == len(keys), f"{tag}: duplicate keypoints"
    missing = [i for i, key in enumerate(keys) if key not in index]
    assert not missing, f"{tag}: {len(missing)} of {len(keys)} keypoints are not the oracle's, first {gk[missing[:3]]}"
    assert 0 < len(keys) <= len(ok), (tag, len(keys), len(ok))
    print(f"{tag}: {len(keys)} of the oracle's {len(ok)} keypoints survive the overflow")
    assert_descriptors(gd, od[[index[key] for key in keys]], tag)


def test_candidate_overflow_clamps_and_leaves_nothing_behind(sift, oracle):
    """61,863 candidates against a capacity of 47,981 (flag 1).  Which ones are stored depends on
    the order of the atomics; every hit is counted, the stored rows fill the capacity exactly and
    are distinct members of the oracle's set, and the results are a subset of the oracle's.  The
    plain frame that follows two flooded ones on the same handle gets a fresh handle's results:
    nothing stale in the counters, the dedupe bitmap or the lists."""
    img, after = tc.flood(), tc.flood_follow_up()
    p = tc.oracle_params(tc.FLOOD)
    kept = tc.extrema_sets(("flood", tc.FLOOD, False), img, p)[1]
    ok, od = tc.oracle_keypoints(("flood", tc.FLOOD, False), img, p)
    _, det = make_detector(sift, tc.FLOOD_W, tc.FLOOD_H, **tc.config_kwargs(tc.FLOOD))
    cap = det.capacities()["candidates"]
    assert len(kept) > cap
    with pytest.warns(sift.SiftCapacityWarning):
        det.detectAndCompute(img)
    for rep in range(2):
        if rep:
            det.detectAndCompute(img)
        cand, hits = det.debug_candidates(return_count=True)
        assert hits == len(kept), (hits, len(kept))
        assert len(cand) == cap
        stored = tc.sort_rows(cand)
        assert not (stored[1:] == stored[:-1]).all(1).any(), "a candidate is stored twice"
        pos = np.searchsorted(_row_keys(kept), _row_keys(stored))
        assert np.array_equal(kept[np.minimum(pos, len(kept) - 1)], stored), "a stored candidate is not the oracle's"
        gk, gd, _ = gpu_keypoints(det)
        assert_overflowed_subset(gk, gd, det.overflow_flags(), ok, od, f"flood run {rep}")

    _, fresh = run(sift, after, tc.FLOOD)
    det.detectAndCompute(after)
    assert det.overflow_flags() == 0 and fresh.overflow_flags() == 0
    assert np.array_equal(tc.sort_rows(det.debug_candidates()), tc.sort_rows(fresh.debug_candidates()))
    for a, b in zip(gpu_keypoints(det), gpu_keypoints(fresh)):
        assert np.array_equal(a, b)
    ak, ad = tc.oracle_keypoints(("follow", tc.FLOOD, False), after, p)
    assert_candidates(det, tc.extrema_sets(("follow", tc.FLOOD, False), after, p)[1], "after the flood")
    assert_results(det, ak, ad, "after the flood")

    # the same sequence through a two-frame batch handle
    with pytest.warns(sift.SiftCapacityWarning):
        bdet, _dev = batch_detect(sift, np.stack([img, img]), tc.FLOOD)
    for i in range(2):
        gk, gd = batch_keypoints(bdet, i)
        assert_overflowed_subset(gk, gd, bdet.batch_results(i)[1], ok, od, f"flood batch frame {i}")
    dev2 = sift.DeviceArray.from_numpy(np.stack([after, after]))
    bdet.detectBatchDevice(dev2.value, 2, tc.FLOOD_W * 4, tc.FLOOD_H * tc.FLOOD_W * 4, sync=True)
    fk, fd, _ = gpu_keypoints(fresh)
    for i in range(2):
        count, flags = bdet.batch_results(i)[:2]
        gk, gd = batch_keypoints(bdet, i)
        assert flags == 0 and count == len(fk), (i, flags, count)
        assert np.array_equal(gk, fk) and np.array_equal(gd, fd), i


def _row_keys(q):
    """(octave, layer, r, c) rows as sortable integers (lexicographic order of sort_rows)."""
    q = q.astype(np.int64)
    return (q[:, 0] << 48) | (q[:, 1] << 40) | (q[:, 2] << 20) | q[:, 3]


# --- 5. flat regions ------------------------------------------------------------------------
FLAT_FRAMES = {"sky": tc.sky, "flat128": lambda: tc.flat(128), "flat255": lambda: tc.flat(255)}


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("case", tc.FLAT_CONFIGS, ids=tc.case_id)
@pytest.mark.parametrize("name", list(FLAT_FRAMES))
def test_flat_regions_do_not_flood(sift, oracle, name, case, u8):
    """thr = 0: OpenCV makes every sample of some layers of a flat non-zero region a candidate
    (rounding residue: 88,286 on the sky frame against a capacity of 31,987) and refines none of
    them.  Before the extrema kernels dropped in-layer-flat hits, every row here but flat 128 at
    3 layers raised flag 1 and the capacity warning (flat 128 at 3 layers: 16,770 candidates,
    half the capacity, for nothing); on the sky frame the stored third of the candidates
    happened to hold the real ones in every run measured, so no keypoint was seen lost."""
    img = FLAT_FRAMES[name]()
    if u8:
        img = img.astype(np.uint8)
    key = (name + ("-u8" if u8 else ""), case, False)
    p = tc.oracle_params(case)
    ok, od = tc.oracle_keypoints(key, img.astype(np.float32), p)
    tag = f"{key[0]} {tc.case_id(case)}"
    _, det = run(sift, img, case)
    assert det.overflow_flags() == 0, f"{tag}: flags {det.overflow_flags()}, {det.total_size} keypoints (oracle {len(ok)})"
    assert_candidates(det, tc.extrema_sets(key, img.astype(np.float32), p)[1], tag)
    assert_results(det, ok, od, tag)
    if name != "sky":
        assert det.total_size == 0 == len(ok)
    else:
        assert len(ok) >= 100
        _, dx = run(sift, img, case, exact_descriptors=True)
        assert_results(dx, ok, od, tag + " exact", exact_mode=True)
