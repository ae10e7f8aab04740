"""Frames and configurations that move the detector off its one operating
point (contrastThreshould 0.04, edgeThreshould 10, a few hundred candidates).

The extrema prefilter is thr = floor(0.5 * ct / L * 255): 0 when ct / L <
0.00784, where every sample that is a 3x3x3 extremum is a candidate.  The
frames here then give candidate lists that are dense (noise), that overrun a
workgroup's LDS list (stripes of period 3: every third column of a layer is
an extremum), that overrun the frame's list (stripes over most of the frame)
or that would, if constant regions counted (sky).  Everything is numpy and
the oracle: test_threshold_cases.py proves each property on the CPU,
test_gpu_thresholds.py relies on it.

A candidate is in-layer-flat when the 3 x 3 block around it in its own DoG
layer is constant.  adjustLocalExtrema can never keep one (all in-layer
derivatives are 0, so the 3 x 3 solve is singular, the iteration stays in
place and the 2-D Hessian's det = 0 fails det > 0), and at thr = 0 the
extrema kernels drop them: the library's candidate set is then the oracle's
minus these (library_candidates).
"""
import numpy as np

import oracle_binding as oracle

# Extrema geometry of another-cuda-sift_amd/csrc/extrema.hip, mirrored:
#   k_extrema_all (L <= 6): a workgroup is four waves over a strip of EX4_COLS
#   = 256 columns; a wave takes 2 rows (EX4_TR = 2), or 12 (6 * kExStream) in
#   launches of many strips, so a workgroup's tile is 256 x 8 or 256 x 48, all
#   L layers of one octave; its LDS list holds EX4_LIST entries, later hits
#   go straight to the frame's list.
#   k_extrema (L > 6): EX_TW x EX_TH = 64 x 16 tiles, list EX_LIST.
EX4_COLS, EX4_LIST = 256, 2048
EX4_ROWS_SHORT, EX4_ROWS_TALL = 4 * 2, 4 * 12
EX_TW, EX_TH, EX_LIST = 64, 16, 512
# launch_extrema_all: an octave streams 12 rows per wave from this many
# 6-row strips per launch (frames of a batch counted).
TALL_MIN_SINGLE, TALL_MIN_BATCH = 2048, 1024
ORDER_SLOT_ENTRIES = 8192  # k_order keeps this many oriented entries in registers


def blob_field(w, h, n, seed, bg=128.0):
    """A `bg` grey frame with n random Gaussian blobs (sigma 1.2-3, +-40..110), clipped to 0..255:
    ~11k keypoints at 1280x960 on 128 grey (OpenCV defaults, no doubled base)."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), bg, np.float32)
    ys, xs = rng.integers(8, h - 8, n), rng.integers(8, w - 8, n)
    sig = rng.uniform(1.2, 3.0, n)
    amp = rng.choice([-1, 1], n) * rng.uniform(40, 110, n)
    yy, xx = np.mgrid[-7:8, -7:8]
    for y, x, sg, a in zip(ys, xs, sig, amp):
        img[y - 7:y + 8, x - 7:x + 8] += a * np.exp(-(xx * xx + yy * yy) / (2 * sg * sg))
    return np.clip(img, 0, 255).astype(np.float32)


def stripes(w, h, period):
    """Vertical square wave (0 / 255), constant down the rows.  Period 3 is a single frequency
    that sigma 1.6 blurs to rounding residue; period 4 is two columns up, two down, whose blurred
    pairs stay equal to the bit, so every sample of the layer where its DoG peaks is an extremum."""
    x = np.arange(w, dtype=np.float64)
    row = 127.5 + 127.5 * np.sign(np.sin(2 * np.pi * x / period + 0.3))
    return np.broadcast_to(row.astype(np.float32), (h, w)).copy()


def noise(w, h, seed):
    """Uniform noise 0..255."""
    return np.random.default_rng(seed).uniform(0, 255, (h, w)).astype(np.float32)


# --- the frames ---------------------------------------------------------------
BLOBS_W, BLOBS_H = 320, 200
NOISE_W, NOISE_H, NOISE_SIGMA = 300, 200, 0.6
FLOOD_W, FLOOD_H = 480, 200


def blobs():
    return blob_field(BLOBS_W, BLOBS_H, 1500, 3)


def spill(period=4):
    """Stripes on rows 0..59, black below, blobs on black below row 90."""
    img = np.zeros((BLOBS_H, BLOBS_W), np.float32)
    img[:60] = stripes(BLOBS_W, 60, period)
    img[90:] = blob_field(BLOBS_W, BLOBS_H, 1500, 3, bg=0.0)[90:]
    return img


def flood(period=4):
    """Stripes in columns 0..329, black, blobs on black right of column 360."""
    img = np.zeros((FLOOD_H, FLOOD_W), np.float32)
    img[:, :330] = stripes(FLOOD_W, FLOOD_H, period)[:, :330]
    img[:, 360:] = blob_field(FLOOD_W, FLOOD_H, 2500, 3, bg=0.0)[:, 360:]
    return img


def flood_follow_up():
    """The plain frame that runs on a handle after flood()."""
    return blob_field(FLOOD_W, FLOOD_H, 2500, 3)


def sky():
    """The blobs frame under a saturated sky: rows 0..129 are 255."""
    img = blobs()
    img[:130] = 255.0
    return img


def flat(value):
    return np.full((BLOBS_H, BLOBS_W), value, np.float32)


# --- configurations: (numOctaveLayers, contrastThreshould, edgeThreshould, sigma) ---
CONTRAST_SWEEP = [(3, ct, 10.0, 1.6) for ct in (0.0, 0.01, 0.04, 0.1, 0.3)]
EDGE_SWEEP = [(3, 0.04, e, 1.6) for e in (0.0, 1.0, 1.5, 2.0, 10.0, 100.0, 1e6)]
# One layer at sigma 1.6 needs an 89-tap blur (plane 3: sigma 11.1), which sift_hip_create refuses
# (63 taps at most): the oracle runs it, the library runs one layer at sigma 1.0 (radii 7, 14, 28).
ONE_LAYER_REFUSED = (1, 0.04, 10.0, 1.6)
LAYER_SWEEP = [(1, 0.04, 10.0, 1.0), (2, 0.0, 10.0, 1.6), (5, 0.03, 10.0, 1.6), (6, 0.04, 10.0, 1.6)]
LAYER_SWEEP_THR = [5, 0, 0, 0]
SWEEP = list(dict.fromkeys(CONTRAST_SWEEP + EDGE_SWEEP + LAYER_SWEEP))
# Flat regions: thr = 0 at a common user setting and at the default ct with 6 layers.
FLAT_CONFIGS = [(3, 0.01, 10.0, 1.6), (3, 0.02, 10.0, 1.6), (6, 0.04, 10.0, 1.6)]
# Period-4 stripes need a base sigma under their own scale (the DoG of a period-4 wave peaks at
# sigma ~ 0.64-0.9): sigma 0.6 puts the peak in layer 5 of 6, 7 of 7 and 2 of 3; 1.6 blurs them away.
SPILL6, SPILL7, FLOOD = (6, 0.04, 10.0, 0.6), (7, 0.04, 10.0, 0.6), (3, 0.04, 10.0, 0.6)
NOISE = (3, 0.0, 10.0, NOISE_SIGMA)


def case_id(case):
    layers, ct, edge, sigma = case
    return f"L{layers}-ct{ct:g}-e{edge:g}-s{sigma:g}"


def prefilter(case):
    """The extrema threshold of a configuration (OpenCV: floor(0.5 * ct / L * 255))."""
    return int(np.floor(0.5 * case[1] / case[0] * 255))


def config_kwargs(case, **kw):
    layers, ct, edge, sigma = case
    return dict(numOctaveLayers=layers, contrastThreshould=ct, edgeThreshould=edge, sigma=sigma, numFeatures=0, **kw)


def oracle_params(case, upscale=False):
    layers, ct, edge, sigma = case
    return oracle.params(nfeatures=0, nOctaveLayers=layers, contrastThreshold=ct, edgeThreshold=edge, sigma=sigma,
                         firstOctave=-1 if upscale else 0)


# --- oracle-side helpers --------------------------------------------------------
def in_layer_flat(img, p, cand):
    """Per candidate row (octave, layer, r, c): is its 3 x 3 block of its own DoG layer constant?
    DoG = planes[1:] - planes[:-1] in float32: the kernels' single rounding."""
    pyr = oracle.gaussian_pyramid(img, p)
    out = np.zeros(len(cand), bool)
    for o, planes in enumerate(pyr):
        sel = np.nonzero(cand[:, 0] == o)[0]
        if not len(sel):
            continue
        dog = planes[1:] - planes[:-1]
        assert dog.dtype == np.float32
        l, r, c = cand[sel, 1], cand[sel, 2], cand[sel, 3]
        blocks = np.stack([dog[l, r + dy, c + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
        out[sel] = blocks.max(0) == blocks.min(0)
    return out


def library_candidates(img, p, cand):
    """The rows of the oracle's candidates `cand` that the library keeps: all of them at a prefilter
    threshold other than 0, those not in-layer-flat at threshold 0."""
    if int(np.floor(0.5 * p.contrastThreshold / p.nOctaveLayers * 255)) != 0:
        return cand
    return cand[~in_layer_flat(img, p, cand)]


def sort_rows(q):
    return q[np.lexsort(q.T[::-1])]


_extrema = {}


def extrema_sets(key, img, p):
    """(oracle candidates, those of them the library keeps), each sorted; computed once per key."""
    if key not in _extrema:
        full = sort_rows(oracle.extrema(img, p))
        kept = library_candidates(img, p, full)
        full.setflags(write=False)
        kept.setflags(write=False)
        _extrema[key] = (full, kept)
    return _extrema[key]


_keypoints = {}


def oracle_keypoints(key, img, p):
    """The oracle's (keypoints, descriptors) of a frame, computed once per key."""
    if key not in _keypoints:
        k, d = oracle.detect_and_compute(img, p, cap=1 << 16)
        k.setflags(write=False)
        d.setflags(write=False)
        _keypoints[key] = (k, d)
    return _keypoints[key]


def worst_tile(cand, tw, th):
    """Largest number of candidates in one tw x th tile of one octave (all layers)."""
    if not len(cand):
        return 0
    key = (cand[:, 0].astype(np.int64) << 40) | ((cand[:, 2] // th).astype(np.int64) << 20) | (cand[:, 3] // tw)
    return int(np.unique(key, return_counts=True)[1].max())


def takes_tall_stream(w, h, frames):
    """Does octave 0 of a w x h frame stream 12 rows per wave in a launch of `frames` frames?"""
    strips = (w + EX4_COLS - 1) // EX4_COLS
    return strips * ((h + 5) // 6) * frames >= (TALL_MIN_BATCH if frames > 1 else TALL_MIN_SINGLE)
