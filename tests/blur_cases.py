"""Configurations that drive the Gaussian blur through every radius.

k_blur is instantiated once per radius R = 1..31, and R selects the row
formula (2R+1 <= 5 or not), the LDS layout (R <= 8, 9..24, > 24) and whether
the 16-byte interior staging exists; the pyramid tail pads every plane's taps
to a radius class 4, 8, 13 or 16 and takes an octave only when every layer
radius is <= 16.  A configuration (sigma, numOctaveLayers, upscale) fixes the
radii: R = taps >> 1, taps = cvRound(8 s + 1) | 1 for each blur's s.

The tap counts here come from the oracle (oracle_binding.gaussian_taps), the
reference, not from the library under test; the sigma chain is OpenCV's
(createInitialImage / buildGaussianPyramid, in their float / double
arithmetic).  test_blur_cases.py proves what the table covers;
test_gpu_blur_sweep.py runs it.
"""
import numpy as np

import oracle_binding as oracle

MAX_RADIUS = 31   # kMaxTaps = 63 (sift_kernels.h); sift_hip_create refuses more
TAIL_RMAX = 16    # the pyramid tail takes an octave only if every layer radius is <= 16
TAIL_CLASSES = (4, 8, 13, 16)
TAIL_MAX_LAYERS = 6  # ... and the octave has at most 9 planes

# The sweep frame: ragged in both directions against the 64 x 64 blur tile,
# 4 x 4 tiles (tile (1, 1) is interior for every R <= 31: 128 + 32 <= 197),
# octaves 201, 100, 50, 25, 12, 6 wide.
SWEEP_W, SWEEP_H, SWEEP_FRAME = 201, 197, 31

# (sigma, numOctaveLayers, upscale)
CASES = [
    (3.05, 6, False),  # layers 6..14 (tail class 16), initial 12
    (4.7, 4, False),   # 12, 15, 17, 21, 24, 29
    (5.0, 4, False),   # 13, 16, 18, 22, 26, 31
    (0.45, 2, False),  # 2, 3, 4, 5 (tail class 8), initial 1
    (3.65, 3, False),  # 11, 14, 18, 23, 28
    (4.8, 4, False),   # 13, 15, 18, 21, 25, 30
    (2.35, 2, False),  # 10, 14, 19, 27
    (0.6, 9, False),   # 1 x 4, 2 x 7: the small row formula in k_blur only (12 planes: no tail)
    (1.0, 1, False),   # 7, 14, 28; one layer
    (1.6, 5, False),   # 4, 4, 5, 6, 7, 7, 9 (tail class 13); five layers
    (1.0, 3, True),    # 3, 4, 5, 6, 8; doubled base: initial blur sigma 0.1 -> radius 1
    (0.5, 6, False),   # 1, 1, 2 x 5, 3 (tail class 4): the tail's small row formula, initial 1
    (4.3, 5, False),   # 10, 11, 13, 15, 17, 20, 23
]


# The one-reflection shortcut of the blur's border staging (W > R + 1 and H >
# R + 1, per plane's own radius): one configuration per LDS layout class (max
# radius <= 8, 9..24, > 24), each without the tail (more than 6 layers, or a
# radius > 16), so k_blur itself gets the tiny planes.
ONE_BOUNCE_CASES = [(0.6, 9, False), (4.3, 5, False), (5.0, 4, False)]
# The four-wave blur instantiations run only at >= 2048 tiles per launch.
FOUR_WAVE_CASE = (3.05, 6, False)
# Float frames with negative pixels: a tail configuration whose planes are zero-padded to class 16.
NEGATIVE_CASE = (3.05, 6, False)


def one_bounce_sizes(case):
    """(W, H) straddling the shortcut's condition for the case's smallest and largest radius."""
    init, layers = radii(case)
    out = []
    for r in (min(layers + [init]), max(layers + [init])):
        for wh in ((r + 1, r + 2), (r + 2, r + 1), (r + 2, r + 2), (2 * r + 3, r + 1)):
            if wh not in out:
                out.append(wh)
    return out


def case_id(case):
    sigma, layers, upscale = case
    return f"s{sigma}-L{layers}" + ("-up" if upscale else "")


def radius(sigma):
    """Blur radius of OpenCV's GaussianBlur(sigma) on a float image, from the oracle's taps."""
    n = len(oracle.gaussian_taps(float(sigma)))
    assert n % 2 == 1
    return n >> 1


def blur_sigmas(sigma, layers, upscale):
    """(initial blur's sigma, [layer blur sigmas, planes 1 .. layers + 2])."""
    s = np.float32(sigma)
    init = np.sqrt(np.maximum(s * s - np.float32(0.5) * np.float32(0.5) * np.float32(4 if upscale else 1),
                              np.float32(0.01)), dtype=np.float32)
    k = 2.0 ** (1.0 / layers)
    sig = []
    for i in range(1, layers + 3):
        prev = k ** (i - 1) * sigma
        total = prev * k
        sig.append(float(np.sqrt(total * total - prev * prev)))
    return float(init), sig


def radii(case):
    """(initial-blur radius, [layer radii])."""
    init, sig = blur_sigmas(*case)
    return radius(init), [radius(s) for s in sig]


def tail_class(layer_radii):
    """The tail's padded radius class for these layer radii (numOctaveLayers + 2 of them), or None
    when the tail does not run."""
    m = max(layer_radii)
    if m > TAIL_RMAX or len(layer_radii) - 2 > TAIL_MAX_LAYERS:
        return None
    return next(c for c in TAIL_CLASSES if m <= c)


def config_kwargs(case, **kw):
    sigma, layers, upscale = case
    return dict(sigma=sigma, numOctaveLayers=layers, upscale=upscale, numFeatures=0, **kw)


def oracle_params(case, **kw):
    sigma, layers, upscale = case
    return oracle.params(nfeatures=0, nOctaveLayers=layers, sigma=sigma, firstOctave=-1 if upscale else 0, **kw)


_frames = {}
_keypoints = {}


def sweep_frame(sift, offset=0.0):
    """The sweep frame (read-only, shared); offset -128 gives a float frame with negative pixels."""
    key = float(offset)
    if key not in _frames:
        img = sift.synth_frame(SWEEP_FRAME, SWEEP_W, SWEEP_H) + np.float32(offset)
        img.setflags(write=False)
        _frames[key] = img
    return _frames[key]


def oracle_keypoints(sift, case, offset=0.0):
    """The oracle's (keypoints, descriptors) of a case on the sweep frame, computed once."""
    key = (case, float(offset))
    if key not in _keypoints:
        k, d = oracle.detect_and_compute(sweep_frame(sift, offset), oracle_params(case), cap=1 << 16)
        k.setflags(write=False)
        d.setflags(write=False)
        _keypoints[key] = (k, d)
    return _keypoints[key]
