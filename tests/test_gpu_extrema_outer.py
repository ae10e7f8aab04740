"""k_extrema_all streams the planes G1 .. G(L+1) only.  Layers 1 and L are first
tested against the inner DoG layers (a provisional hit) and then, when the
workgroup's list is flushed or a hit spills past it, against the nine values of
the outer layer (D0 for layer 1, D(L+1) for layer L) loaded around the hit.

The candidate set must be the oracle's at every layer count that takes another
shape of that rule (L = 1: the one layer needs both outer layers; L = 2: both
layers provisional; L = 6: the widest hit word, and thr = 0), in the 2-row and
the 12-row streams, and where provisional hits overrun the LDS list.  The
host model below (numpy on the oracle's pyramid) splits the hits the way the
kernel does, so the tests can show that the outer layers reject something.
"""
import numpy as np
import pytest

import threshold_cases as tc
from test_gpu_parity import make_detector
from test_gpu_thresholds import batch_detect

pytestmark = pytest.mark.gpu

W, H = 300, 200  # a partial second 256-column strip, 25 blocks of 8 rows
FRAME = 2        # sift.synth_frame index (of frames 0..5 the one whose smallest count in test 2 is largest)
LAYERS = (1, 2, 3, 4, 6)
BORDER = 5


def case(layers):
    """Defaults but for the layer count.  One layer at sigma 1.6 needs an 89-tap blur, which the
    library refuses (threshold_cases.ONE_LAYER_REFUSED): it runs at sigma 1.0."""
    return (layers, 0.04, 10.0, 1.0 if layers == 1 else 1.6)


def box3(a, fn):
    """3 x 3 max / min of every interior sample of a (..., H, W) array (the border is left as it is)."""
    out = a.copy()
    v = fn(fn(a[..., :-2, :], a[..., 1:-1, :]), a[..., 2:, :])
    out[..., 1:-1, 1:-1] = fn(fn(v[..., :-2], v[..., 1:-1]), v[..., 2:])
    return out


def row3(a, fn):
    """1 x 3 max / min of every sample of an (H, W) array but the first and last of a row."""
    out = a.copy()
    out[:, 1:-1] = fn(fn(a[:, :-2], a[:, 1:-1]), a[:, 2:])
    return out


def split_hits(img, case_):
    """The kernel's two steps on the oracle's pyramid, rows (octave, layer, r, c).  Returns
    (final, provisional, rejected, hits): `hits` pass the test against the inner layers 1 .. L (what
    a workgroup lists), `provisional` are those of layers 1 and L among them, `rejected` is a dict
    (side, sign) -> the provisional hits that the outer layer of that side ("low": D0, "high":
    D(L+1)) rejects (sign "late": those of both signs that the centre row of the 3 x 3 patch lets
    pass and the row above or below rejects), and `final` = hits minus rejected, sorted."""
    L = case_[0]
    thr = np.float32(tc.prefilter(case_))
    p = tc.oracle_params(case_)
    hits, rejected = [], {(s, g): [] for s in ("low", "high") for g in ("max", "min", "late")}
    for o, planes in enumerate(tc.oracle.gaussian_pyramid(img, p)):
        dog = planes[1:] - planes[:-1]  # float32: the kernels' single rounding
        assert dog.dtype == np.float32 and dog.shape[0] == L + 2
        hx, hn = box3(dog, np.maximum), box3(dog, np.minimum)
        h, w = dog.shape[1:]
        inside = np.zeros((h, w), bool)
        inside[BORDER:h - BORDER, BORDER:w - BORDER] = True
        for l in range(1, L + 1):
            v = dog[l]
            inner = [d for d in (l - 1, l, l + 1) if 1 <= d <= L]
            M, m = hx[inner].max(0), hn[inner].min(0)
            hit = inside & (np.abs(v) > thr) & (v == np.where(v > 0, M, m))
            if thr == 0:  # the kernels drop in-layer-flat hits at thr = 0
                hit &= hx[l] != hn[l]
            bad = np.zeros_like(hit)
            for side, d in (("low", 0), ("high", L + 1)):
                if abs(d - l) != 1:
                    continue
                rmax, rmin = hit & (v > 0) & (hx[d] > v), hit & (v < 0) & (hn[d] < v)
                # the kernel compares the centre row of the patch first, the rows above and below after it
                cx, cn = row3(dog[d], np.maximum), row3(dog[d], np.minimum)
                late = (rmax & ~(cx > v)) | (rmin & ~(cn < v))
                for sign, r in (("max", rmax), ("min", rmin), ("late", late)):
                    rr, cc = np.nonzero(r)
                    rejected[side, sign].append(np.stack([np.full_like(rr, o), np.full_like(rr, l), rr, cc], 1))
                bad |= rmax | rmin
            rr, cc = np.nonzero(hit)
            hits.append(np.stack([np.full_like(rr, o), np.full_like(rr, l), rr, cc, bad[rr, cc]], 1))
    hits = np.concatenate(hits).astype(np.int32)
    final = tc.sort_rows(hits[hits[:, 4] == 0][:, :4])
    provisional = hits[(hits[:, 1] == 1) | (hits[:, 1] == L)][:, :4]
    return final, provisional, {k: np.concatenate(v) for k, v in rejected.items()}, hits[:, :4]


def frame(sift):
    return sift.synth_frame(FRAME, W, H)


# --- 1. layer counts -----------------------------------------------------------------
@pytest.mark.parametrize("layers", LAYERS)
def test_layer_counts(sift, oracle, layers):
    """One ragged frame, auto octaves: candidates equal to the oracle's at L = 1, 2, 3, 4, 6."""
    img, c = frame(sift), case(layers)
    _, det = make_detector(sift, W, H, **tc.config_kwargs(c))
    det.detectAndCompute(img)
    kept = tc.extrema_sets((f"outer{FRAME}", c, False), img, tc.oracle_params(c))[1]
    cand, hits = det.debug_candidates(return_count=True)
    assert det.overflow_flags() == 0
    assert hits == len(cand) == len(kept) > 0, (layers, hits, len(cand), len(kept))
    assert np.array_equal(tc.sort_rows(cand), kept), layers


# --- 2. the outer layers reject something ------------------------------------------------
@pytest.mark.parametrize("layers", LAYERS)
def test_outer_layers_reject_something(sift, oracle, layers):
    """On the frame of test 1 the outer layers reject provisional hits of layer 1 and of layer L,
    maxima and minima, at least 10 of each, and on either side at least 10 only by the rows above
    and below the centre row (the kernel's second step): a kernel that skipped a side, a sign or
    a step would fail test 1.  The host split reproduces the oracle's set, so it counts the right
    thing."""
    img, c = frame(sift), case(layers)
    final, provisional, rejected, _ = split_hits(img, c)
    kept = tc.extrema_sets((f"outer{FRAME}", c, False), img, tc.oracle_params(c))[1]
    assert np.array_equal(final, kept), layers
    counts = {k: len(v) for k, v in rejected.items()}
    print(f"L={layers}: {len(kept)} candidates, {len(provisional)} provisional hits, rejected {counts}")
    assert all(n >= 10 for (_, sign), n in counts.items() if sign != "late"), (layers, counts)
    # one such hit is enough for a skipped second step to change test 1's set
    assert all(n > 0 for (_, sign), n in counts.items() if sign == "late"), (layers, counts)


# --- 3. tall streams -----------------------------------------------------------------------
TALL_W, TALL_H, TALL_N = 320, 208, 16


def test_tall_stream_batch_equals_single_frames(sift, oracle):
    """16 distinct frames in one launch: octave 0 streams 12 rows per wave (2 strips x 35 six-row
    steps x 16 frames >= 1024).  Every frame's results are bit-equal to the same frame through a
    single-frame handle (the 2-row stream of test 1); the constant frame in the middle of the batch
    has no candidate and inherits none."""
    assert tc.takes_tall_stream(TALL_W, TALL_H, TALL_N) and not tc.takes_tall_stream(TALL_W, TALL_H, 1)
    frames = np.stack([sift.synth_frame(i, TALL_W, TALL_H) for i in range(TALL_N)])
    flat_at = 7
    frames[flat_at] = 128.0
    c = case(3)
    det, _dev = batch_detect(sift, frames, c)
    _, one = make_detector(sift, TALL_W, TALL_H, **tc.config_kwargs(c))
    for i in range(TALL_N):
        one.detectAndCompute(frames[i])
        one.copyToHost(True)
        count, flags = det.batch_results(i)[:2]
        k3, f4, d = det.batch_copy_to_host(i)
        assert flags == 0 and one.overflow_flags() == 0, (i, flags)
        assert count == one.total_size, (i, count, one.total_size)
        assert (count == 0) == (i == flat_at), (i, count)
        assert np.array_equal(k3.view(np.uint32), one.final_kpts.view(np.uint32)), i
        assert np.array_equal(f4.view(np.uint32), one.final_features.view(np.uint32)), i
        assert np.array_equal(d.view(np.uint16), one.descriptors.view(np.uint16)), i


# --- 4. spill path -------------------------------------------------------------------------
SPILL_SEED, SPILL_CASE = 0, (6, 0.04, 10.0, 0.85)  # thr = floor(0.5 * 0.04 / 6 * 255) = 0
SPILL_WORST_BLOCK = 2247  # hits (provisional and final) in the fullest 256 x 48 block of octave 0, seed 0


def int_noise(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.float32)


def test_provisional_hits_spill_past_the_lds_list(sift, oracle):
    """Integer noise 0..255 at 6 layers and sigma 0.85, 16 frames in one launch so that octave 0
    takes the 12-row stream (blocks of 256 x 48): frame 0 lists 12,604 hits, 2,247 of them in its
    fullest block against a list of 2,048, and the outer layers reject 583 of the 12,604 (sigma 0.6
    fills the blocks further, 2,986, but rejects none; at sigma 1.0 no block passes 1,627).  Hits past
    the list are resolved one by one on their way to the frame's list."""
    assert tc.prefilter(SPILL_CASE) == 0 and tc.takes_tall_stream(W, H, 16)
    frames = np.stack([int_noise(SPILL_SEED + i) for i in range(16)])
    final, _, rejected, hits = split_hits(frames[0], SPILL_CASE)
    kept = tc.extrema_sets(("outer-spill", SPILL_CASE, False), frames[0], tc.oracle_params(SPILL_CASE))[1]
    assert np.array_equal(final, kept)
    worst = tc.worst_tile(hits[hits[:, 0] == 0], tc.EX4_COLS, tc.EX4_ROWS_TALL)
    assert worst == SPILL_WORST_BLOCK > tc.EX4_LIST
    assert sum(len(v) for (_, sign), v in rejected.items() if sign != "late") >= 500
    det, _dev = batch_detect(sift, frames, SPILL_CASE, maxKeypoints=32768)
    assert len(kept) < det.capacities()["candidates"]
    cand, count = det.debug_candidates(return_count=True)  # frame 0 of the batch
    assert det.batch_results(0)[1] == 0
    assert count == len(cand) == len(kept), (count, len(cand), len(kept))
    assert np.array_equal(tc.sort_rows(cand), kept)
