"""The frame-launch path seen from its entry points ("Frame launch").

Two pins under the host orchestration of libsift_hip.so (detector.hip, lanes.hip):

1. Argument errors: every entry point that takes a frame, given every defect that applies to it -- and two at once,
   which pins the order of the checks -- returns the status code and the exact sift_hip_last_error text recorded
   here, and launches nothing.
2. Every kind of frame on one handle -- graph replay with the cached and the re-pointed head, a changed pitch, a
   masked frame, caller-supplied keypoints, host frames, pipelined submits -- gives, frame by frame, the bits of the
   same calls made synchronously on a fresh one-lane handle, prev_descriptor included; again on a batch handle,
   whose single-frame graphs and partial batch run there.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_input import assert_identical, results
from test_gpu_lanes import prev_rows
from test_gpu_mask import half_plane
from test_gpu_parity import make_detector

pytestmark = pytest.mark.gpu

W, H = 752, 480
F32, U8, BAD_FMT = 0, 1, 7
INVALID = -1  # SIFT_HIP_ERR_INVALID

NULL_IMAGE = "null image"
NULL_FRAMES = "null frames"
FORMAT = "unknown pixel format"
DEV_STRIDE = "row stride must be a multiple of the pixel size and >= width"
HOST_STRIDE = "row stride smaller than width"
FRAME_COUNT = "frame count outside 1..batch capacity"
FRAME_STRIDE = "frame stride smaller than one frame"
MASK_STRIDE = "mask row stride smaller than width"
MASK_FRAME_STRIDE = "mask frame stride smaller than one mask"
NEGATIVE_COUNT = "negative keypoint count"
NULL_KEYPOINTS = "null keypoints"


def error_cases(L, h, img, img8, mask, kpts, himg, himg8, hmask, hkpts, cap):
    """(label, call, expected message).  img / img8 / mask / kpts: device pointers of two f32 frames, two u8 frames,
    two masks and a few valid keypoints; h*: the same on the host; cap: the result capacity."""
    above = f"keypoint count {cap + 1} above the result capacity {cap} (sift_hip_capacities)"
    row, row8 = 4 * W, W
    t = ctypes.c_longlong()
    tk = ctypes.byref(t)
    nk = len(hkpts)
    c = []

    def add(label, msg, fn, *args):
        c.append((label, lambda: fn(h, *args), msg))

    fn = L.sift_hip_detect_device_fmt  # (img, stride, format, stream)
    add("detect_device_fmt: null image", NULL_IMAGE, fn, None, row, F32, None)
    add("detect_device_fmt: unknown format", FORMAT, fn, img, row, BAD_FMT, None)
    add("detect_device_fmt: f32 stride below width", DEV_STRIDE, fn, img, row - 4, F32, None)
    add("detect_device_fmt: u8 stride below width", DEV_STRIDE, fn, img8, row8 - 1, U8, None)
    add("detect_device_fmt: f32 stride not a multiple of 4", DEV_STRIDE, fn, img, row + 2, F32, None)
    add("detect_device_fmt: null image + unknown format", NULL_IMAGE, fn, None, row, BAD_FMT, None)
    add("detect_device_fmt: unknown format + stride below width", FORMAT, fn, img, 1, BAD_FMT, None)

    fn = L.sift_hip_detect_device_masked  # (img, stride, format, mask, mask_stride, stream)
    add("detect_device_masked: null image", NULL_IMAGE, fn, None, row, F32, mask, W, None)
    add("detect_device_masked: unknown format", FORMAT, fn, img, row, BAD_FMT, mask, W, None)
    add("detect_device_masked: stride below width", DEV_STRIDE, fn, img, row - 4, F32, mask, W, None)
    add("detect_device_masked: stride not a multiple of 4", DEV_STRIDE, fn, img, row + 1, F32, mask, W, None)
    add("detect_device_masked: mask stride below width", MASK_STRIDE, fn, img, row, F32, mask, W - 1, None)
    add("detect_device_masked: stride + mask stride", DEV_STRIDE, fn, img, row - 4, F32, mask, W - 1, None)
    add("detect_device_masked: null image + mask stride", NULL_IMAGE, fn, None, row, F32, mask, W - 1, None)

    fn = L.sift_hip_detect_batch_device  # (frames, n, stride, frame_stride, format, stream)
    add("detect_batch_device: null frames", NULL_FRAMES, fn, None, 2, row, 0, F32, None)
    add("detect_batch_device: n = 0", FRAME_COUNT, fn, img, 0, row, 0, F32, None)
    add("detect_batch_device: n = B + 1", FRAME_COUNT, fn, img, 3, row, 0, F32, None)
    add("detect_batch_device: unknown format", FORMAT, fn, img, 2, row, 0, BAD_FMT, None)
    add("detect_batch_device: stride below width", DEV_STRIDE, fn, img, 2, row - 4, 0, F32, None)
    add("detect_batch_device: stride not a multiple of 4", DEV_STRIDE, fn, img, 2, row + 2, 0, F32, None)
    add("detect_batch_device: frame stride too small", FRAME_STRIDE, fn, img, 2, row, row * H - 4, F32, None)
    add("detect_batch_device: u8 frame stride too small", FRAME_STRIDE, fn, img8, 2, row8, row8 * H - 1, U8, None)
    add("detect_batch_device: null frames + n = 0", NULL_FRAMES, fn, None, 0, row, 0, F32, None)
    add("detect_batch_device: n = B + 1 + unknown format", FRAME_COUNT, fn, img, 3, row, 0, BAD_FMT, None)
    add("detect_batch_device: stride + frame stride", DEV_STRIDE, fn, img, 2, row - 4, 8, F32, None)

    fn = L.sift_hip_detect_batch_device_masked  # (frames, n, stride, frame_stride, format, masks, mask_stride, mask_frame_stride, stream)
    add("detect_batch_device_masked: null frames", NULL_FRAMES, fn, None, 2, row, 0, F32, mask, W, 0, None)
    add("detect_batch_device_masked: n = 0", FRAME_COUNT, fn, img, 0, row, 0, F32, mask, W, 0, None)
    add("detect_batch_device_masked: n = B + 1", FRAME_COUNT, fn, img, 3, row, 0, F32, mask, W, 0, None)
    add("detect_batch_device_masked: unknown format", FORMAT, fn, img, 2, row, 0, BAD_FMT, mask, W, 0, None)
    add("detect_batch_device_masked: stride below width", DEV_STRIDE, fn, img, 2, row - 4, 0, F32, mask, W, 0, None)
    add("detect_batch_device_masked: frame stride too small", FRAME_STRIDE, fn, img, 2, row, row * H - 4, F32, mask, W, 0, None)
    add("detect_batch_device_masked: mask stride below width", MASK_STRIDE, fn, img, 2, row, 0, F32, mask, W - 1, 0, None)
    add("detect_batch_device_masked: mask frame stride too small", MASK_FRAME_STRIDE, fn, img, 2, row, 0, F32, mask, W, W * H - 1, None)
    add("detect_batch_device_masked: frame stride + mask stride", FRAME_STRIDE, fn, img, 2, row, 8, F32, mask, W - 1, 0, None)
    add("detect_batch_device_masked: mask stride + mask frame stride", MASK_STRIDE, fn, img, 2, row, 0, F32, mask, W - 1, 8, None)

    fn = L.sift_hip_submit_device  # (img, stride, format, stream, ticket)
    add("submit_device: null image", NULL_IMAGE, fn, None, row, F32, None, tk)
    add("submit_device: unknown format", FORMAT, fn, img, row, BAD_FMT, None, tk)
    add("submit_device: stride below width", DEV_STRIDE, fn, img, row - 4, F32, None, tk)
    add("submit_device: stride not a multiple of 4", DEV_STRIDE, fn, img, row + 3, F32, None, tk)
    add("submit_device: null image + unknown format", NULL_IMAGE, fn, None, row, BAD_FMT, None, tk)

    fn = L.sift_hip_compute_device  # (img, stride, format, dev_kpts, n, stream)
    add("compute_device: null image", NULL_IMAGE, fn, None, row, F32, kpts, nk, None)
    add("compute_device: unknown format", FORMAT, fn, img, row, BAD_FMT, kpts, nk, None)
    add("compute_device: stride below width", DEV_STRIDE, fn, img, row - 4, F32, kpts, nk, None)
    add("compute_device: stride not a multiple of 4", DEV_STRIDE, fn, img, row + 2, F32, kpts, nk, None)
    add("compute_device: negative count", NEGATIVE_COUNT, fn, img, row, F32, kpts, -1, None)
    add("compute_device: count above capacity", above, fn, img, row, F32, kpts, cap + 1, None)
    add("compute_device: null keypoints", NULL_KEYPOINTS, fn, img, row, F32, None, nk, None)
    add("compute_device: stride + count above capacity", DEV_STRIDE, fn, img, row - 4, F32, kpts, cap + 1, None)
    add("compute_device: count above capacity + null keypoints", above, fn, img, row, F32, None, cap + 1, None)

    # Host frames: the format is checked before the image, and the stride only against the width.
    add("detect: null image", NULL_IMAGE, L.sift_hip_detect, None, row)
    add("detect: stride below width", HOST_STRIDE, L.sift_hip_detect, himg, row - 1)
    add("detect: null image + stride below width", NULL_IMAGE, L.sift_hip_detect, None, 4)
    add("detect_u8: null image", NULL_IMAGE, L.sift_hip_detect_u8, None, row8)
    add("detect_u8: stride below width", HOST_STRIDE, L.sift_hip_detect_u8, himg8, row8 - 1)

    fn = L.sift_hip_submit  # (img, stride, format, ticket)
    add("submit: null image", NULL_IMAGE, fn, None, row, F32, tk)
    add("submit: unknown format", FORMAT, fn, himg, row, BAD_FMT, tk)
    add("submit: stride below width", HOST_STRIDE, fn, himg, row - 4, F32, tk)
    add("submit: u8 stride below width", HOST_STRIDE, fn, himg8, row8 - 1, U8, tk)
    add("submit: null image + unknown format", FORMAT, fn, None, row, BAD_FMT, tk)

    fn = L.sift_hip_detect_masked  # (img, stride, format, mask, mask_stride)
    add("detect_masked: null image", NULL_IMAGE, fn, None, row, F32, hmask, W)
    add("detect_masked: unknown format", FORMAT, fn, himg, row, BAD_FMT, hmask, W)
    add("detect_masked: stride below width", HOST_STRIDE, fn, himg, row - 4, F32, hmask, W)
    add("detect_masked: mask stride below width", MASK_STRIDE, fn, himg, row, F32, hmask, W - 1)
    add("detect_masked: null image + mask stride", MASK_STRIDE, fn, None, row, F32, hmask, W - 1)
    add("detect_masked: unknown format + mask stride", FORMAT, fn, himg, row, BAD_FMT, hmask, W - 1)
    add("detect_masked: no mask, null image", NULL_IMAGE, fn, None, row, F32, None, 0)
    add("detect_masked: no mask, unknown format + null image", FORMAT, fn, None, row, BAD_FMT, None, 0)

    fn = L.sift_hip_compute  # (img, stride, kpts, n): the keypoints are checked before the image
    add("compute: count above capacity", above, fn, himg, row, hkpts.ctypes.data, cap + 1)
    add("compute: null keypoints", NULL_KEYPOINTS, fn, himg, row, None, nk)
    add("compute: null image + count above capacity", above, fn, None, row, hkpts.ctypes.data, cap + 1)
    add("compute: null image", NULL_IMAGE, fn, None, row, hkpts.ctypes.data, nk)
    add("compute: stride below width", HOST_STRIDE, fn, himg, row - 4, hkpts.ctypes.data, nk)
    return c


def test_argument_errors_are_pinned(sift):
    from sift_amd import cv

    L = sift.lib()
    A, B = sift.synth_frame(31, W, H), sift.synth_frame(32, W, H)
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3)
    fresh = sift.Detector(cfg, lanes=1)
    fresh.detectAndCompute(A)
    ref = results(fresh)
    assert len(ref[0]) > 100

    det = sift.Detector(cfg, batch=2)
    det.gpuWarmUpAndAllocate()
    himg = np.stack([A, B])
    himg8 = himg.astype(np.uint8)
    hmask = np.stack([half_plane(W, H), half_plane(W, H, left=False)])
    hkpts = cv.keypoint_records(ref[0], ref[1])[:16].copy()
    assert det.check_keypoints(hkpts) == -1
    img, img8, mask, kpts = (sift.DeviceArray.from_numpy(a) for a in (himg, himg8, hmask, hkpts))
    cap = det.capacities()["results"]

    def count():
        n = ctypes.c_int(-1)
        assert L.sift_hip_num_keypoints(det.handle, ctypes.byref(n)) == 0
        return n.value

    det.detectAndCompute(B)
    t0 = det.submitDevice(img.value, 4 * W)
    det.wait(t0)
    n0 = count()
    assert n0 == len(ref[0]) == det.total_size

    cases = error_cases(L, det.handle, img.value, img8.value, mask.value, kpts.value, himg.ctypes.data,
                        himg8.ctypes.data, hmask.ctypes.data, hkpts, cap)
    assert len(cases) >= 70 and len({label for label, _, _ in cases}) == len(cases)
    wrong = []
    for label, call, msg in cases:
        rc = call()
        got = L.sift_hip_last_error().decode()
        print(f"{label}: {rc} {got!r}")
        if rc != INVALID or got != msg:
            wrong.append((label, rc, got, msg))
    assert not wrong, wrong

    # Nothing was launched: no frame number was taken, the current frame is still the one before the errors, and the
    # handle goes on as a fresh one does.
    assert count() == n0
    assert_identical(results(det), ref)
    t1 = det.submitDevice(img.value + A.nbytes, 4 * W)
    assert t1 == t0 + 1
    det.wait(t1)
    det.detectAndCompute(A)
    assert det.total_size == n0
    assert_identical(results(det), ref)


def snapshot(sift, det):
    """The current frame's results, prev_size and the prev_descriptor rows."""
    return results(det) + (np.array([det.prev_size]), prev_rows(sift, det, det.prev_size))


class Buffers:
    """The inputs of the frame sequence: device frames A, B, a strided copy of A, a device mask and device keypoints;
    their host counterparts."""

    def __init__(self, sift, kpts_of):
        self.A, self.B = sift.synth_frame(41, W, H), sift.synth_frame(42, W, H)
        self.pitch = W + 16
        wide = np.zeros((H, self.pitch), np.float32)
        wide[:, :W] = self.A
        self.A8 = self.A.astype(np.uint8)
        self.mask = half_plane(W, H)
        self.kpts = kpts_of(self.A)
        self.dA, self.dB, self.dWide, self.dA8, self.dMask, self.dKpts = (
            sift.DeviceArray.from_numpy(a) for a in (self.A, self.B, wide, self.A8, self.mask, self.kpts))
        self.pipelined = [sift.synth_frame(43 + i, W, H) for i in range(5)]
        self.dPipelined = [sift.DeviceArray.from_numpy(f) for f in self.pipelined]


def device_steps(b, batch):
    """The device part of the sequence as (name, call on a detector); `batch`: the handle takes frame batches."""
    row = 4 * W
    steps = [
        ("detect_device(A)", lambda d: d.detectAndComputeDevice(b.dA.value, row)),
        ("detect_device(A), cached head", lambda d: d.detectAndComputeDevice(b.dA.value, row)),
        ("detect_device(B), head re-pointed", lambda d: d.detectAndComputeDevice(b.dB.value, row)),
        ("detect_device(strided A)", lambda d: d.detectAndComputeDevice(b.dWide.value, 4 * b.pitch)),
        ("detect_device(u8 A)", lambda d: d.detectAndComputeDevice(b.dA8.value, W, u8=True)),
        ("detect_device_masked(A)", lambda d: d.detectAndComputeDevice(b.dA.value, row, mask_ptr=b.dMask.value)),
        ("compute_device(A)", lambda d: d.computeDevice(b.dA.value, row, b.dKpts.value, len(b.kpts))),
    ]
    if batch:  # a batch of one frame takes the single-frame graph, as the detect_device calls on this handle do
        steps.append(("detect_batch_device(B, 1)", lambda d: (d.detectBatchDevice(b.dB.value, 1, row) if d.batch > 1
                                                              else d.detectAndComputeDevice(b.dB.value, row))))
    return steps


def host_steps(b):
    return [
        ("detect_u8", lambda d: d.detectAndCompute(b.A8)),
        ("detect_masked", lambda d: d.detectAndCompute(b.B, b.mask)),
        ("compute", lambda d: d.compute(b.A, b.kpts)),
    ]


def run_steps(sift, det, steps):
    out = []
    for name, call in steps:
        call(det)
        out.append((name, snapshot(sift, det)))
    return out


def run_submits(sift, det, b, depth):
    """The five pipelined frames through submit_device, `depth` in flight (1: each waited at once)."""
    out, queue = [], []
    for i, f in enumerate(b.dPipelined):
        queue.append(det.submitDevice(f.value, 4 * W))
        if len(queue) == depth:
            det.wait(queue.pop(0))
            out.append((f"submit_device {len(out)}", snapshot(sift, det)))
    while queue:
        det.wait(queue.pop(0))
        out.append((f"submit_device {len(out)}", snapshot(sift, det)))
    return out


def assert_same_frames(got, ref):
    assert [name for name, _ in got] == [name for name, _ in ref]
    for (name, g), (_, r) in zip(got, ref):
        assert len(g[0]) == len(r[0]), f"{name}: {len(g[0])} keypoints, expected {len(r[0])}"
        assert g[3][0] == r[3][0], f"{name}: prev_size {g[3][0]}, expected {r[3][0]}"
        for what, x, y in zip(("kpts3", "feats4", "descriptors", "prev_size", "prev_descriptor"), g, r):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{name}: {what} differ"


@pytest.fixture(scope="module")
def buffers(sift):
    from sift_amd import cv

    def kpts_of(frame):
        _, det = make_detector(sift, W, H, numOctaves=3, lanes=1)
        det.detectAndCompute(frame)
        k3, f4, _ = results(det)
        kp = cv.keypoint_records(k3, f4)[::3].copy()
        assert len(kp) > 100 and det.check_keypoints(kp) == -1
        return kp

    return Buffers(sift, kpts_of)


def sequence(sift, det, b, depth, batch, host):
    last = [("detect_device(A), after the submits", lambda d: d.detectAndComputeDevice(b.dA.value, 4 * W))]
    out = run_steps(sift, det, device_steps(b, batch))
    if host:
        out += run_steps(sift, det, host_steps(b))
    out += run_submits(sift, det, b, depth)
    return out + run_steps(sift, det, last)


def test_every_frame_kind_on_one_handle(sift, buffers):
    _, ref = make_detector(sift, W, H, numOctaves=3, lanes=1)
    expected = sequence(sift, ref, buffers, 1, batch=False, host=True)
    assert ref.lanes() == (1, 1)
    assert len(expected) == 16 and all(len(s[0]) > 100 for _, s in expected)
    kinds = dict(expected)
    assert len(kinds["detect_device_masked(A)"][0]) < len(kinds["detect_device(A)"][0])
    assert len(kinds["compute_device(A)"][0]) == len(buffers.kpts)
    _, det = make_detector(sift, W, H, numOctaves=3, lanes=3)
    assert_same_frames(sequence(sift, det, buffers, 3, batch=False, host=True), expected)
    assert det.lanes()[1] > 1  # the submits ran on more than one lane


def test_device_frame_kinds_on_a_batch_handle(sift, buffers):
    """On a set_batch(2) handle every single frame takes the lane's single-frame graphs, and a batch of one frame
    with them; a full batch's frames are the single frames' results."""
    b = buffers
    _, ref = make_detector(sift, W, H, numOctaves=3, lanes=1)
    expected = sequence(sift, ref, b, 1, batch=True, host=False)
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3)
    det = sift.Detector(cfg, batch=2, lanes=3)
    det.gpuWarmUpAndAllocate()
    assert_same_frames(sequence(sift, det, b, 3, batch=True, host=False), expected)
    # a full batch (A, B): frame i's results are those of the single frames above
    both = sift.DeviceArray.from_numpy(np.stack([b.A, b.B]))
    det.detectBatchDevice(both.value, 2, 4 * W)
    assert det.batch_frames() == 2
    kinds = dict(expected)
    for i, name in enumerate(("detect_device(A)", "detect_device(B), head re-pointed")):
        k3, f4, desc = det.batch_copy_to_host(i)
        assert_identical((k3, f4, desc.view(np.uint16)), kinds[name][:3])
