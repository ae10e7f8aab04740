"""RootSIFT on the GPU: the detector norm (Detector(root_sift=True), sift_hip_set_descriptor_norm) fused into both
descriptor kernels, and the stand-alone transform (sift_amd.rootsift_device / rootsift).

One bar everywhere, no tolerance: the rule is total and integer-in, integer-out (include/sift_hip.h), so every root
row equals sift_amd.cv.rootsift of the row the same call writes without the norm, byte for byte, and keypoints are
untouched.  256 x 256 frames."""
import os
import warnings

import numpy as np
import pytest

from parity_bar import assert_descriptor_bar
from test_gpu_golden import config_for
from test_gpu_parity import assert_same_keypoints, gpu_keypoints, sort_keys

pytestmark = pytest.mark.gpu
W = H = 256
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    import json

    with np.load(os.path.join(GOLD, "camera256.npz"), allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    with open(os.path.join(GOLD, "golden.json")) as f:
        return data, json.load(f)


def make(sift, root, exact=False, **kw):
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numFeatures=0)
    det = sift.Detector(cfg, exact_descriptors=exact, root_sift=root, **kw)
    det.gpuWarmUpAndAllocate()
    return det


def rows(det):
    """(kpts3 bytes, feats4 bytes, descriptor rows as uint8) of the current frame; every row entry must be a byte."""
    det.copyToHost(True)
    d = det.descriptors.astype(np.float32)
    assert np.array_equal(d, np.rint(d)) and (d >= 0).all() and (d <= 255).all()
    return det.final_kpts.tobytes(), det.final_features.tobytes(), d.astype(np.uint8)


def d2h(sift, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    if out.size:
        sift._check(sift.lib().sift_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "d2h")
    return out


def device_bytes(sift, ptr, n):
    return d2h(sift, ptr, (n, 128), np.uint16).view(np.float16).astype(np.float32).astype(np.uint8)


# ---- golden, exact mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "base_n60"])
def test_golden_exact_root(sift, gold, name):
    """Fails without the feature: no GPU-side reference, the golden bytes through the numpy mirror."""
    from sift_amd import cv

    data, meta = gold
    det = sift.Detector(config_for(sift, meta["configs"][name]), exact_descriptors=True, root_sift=True)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(data["camera256"].astype(np.float32))
    gk, gd, _ = gpu_keypoints(det)
    ok, od = data[f"{name}_kpts"], cv.rootsift(data[f"{name}_desc"])
    assert_same_keypoints(gk, ok)
    assert np.array_equal(gd[sort_keys(gk)], od[sort_keys(ok)].astype(np.float32))


# ---- fixed-point mode: plain against root, single frame (k_descriptor<256>) and batch (k_descriptor<128>) --------------
@pytest.fixture(scope="module")
def frames(sift):
    f = [sift.synth_frame(i, W, H) for i in (1, 2, 3)]
    for a in f:
        a.flags.writeable = False
    return f


@pytest.fixture(scope="module")
def single(sift, frames):
    """Per descriptor mode and frame: the plain rows and the root rows of single-frame calls (computed once)."""
    out = {}
    for exact in (False, True):
        plain, root = make(sift, False, exact), make(sift, True, exact)
        for i, img in enumerate(frames):
            plain.detectAndCompute(img)
            root.detectAndCompute(img)
            out[exact, i] = rows(plain), rows(root)
    return out


@pytest.mark.parametrize("exact", [False, True])
def test_single_frame_plain_against_root(sift, single, frames, exact):
    from sift_amd import cv

    for i in range(len(frames)):
        (pk, pf, pd), (rk, rf, rd) = single[exact, i]
        assert len(pd) > 50 and pk == rk and pf == rf, "keypoints differ between the norms"
        bad = np.nonzero((rd != cv.rootsift(pd)).any(axis=1))[0]
        assert len(bad) == 0, f"frame {i}: {len(bad)} of {len(pd)} rows differ from cv.rootsift(plain), first {bad[:5]}"
        assert not np.array_equal(rd, pd)


@pytest.mark.parametrize("exact", [False, True])
def test_batch_equals_single(sift, single, frames, exact):
    det = make(sift, True, exact, batch=3)
    dev = sift.DeviceArray.from_numpy(np.stack(frames))
    det.detectBatchDevice(dev.value, 3, W * 4, W * H * 4)
    assert det.batch_frames() == 3
    for i in range(3):
        k3, f4, d = det.batch_copy_to_host(i)
        rk, rf, rd = single[exact, i][1]
        assert k3.tobytes() == rk and f4.tobytes() == rf, i
        assert np.array_equal(d.astype(np.float32), rd.astype(np.float32)), i
    # a single-frame call on the batch handle (frame 0's arena, the one-frame graph)
    det.detectAndCompute(frames[1])
    assert rows(det)[2].tobytes() == single[exact, 1][1][2].tobytes()


# ---- every path that launches the descriptor kernel carries the norm ---------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_every_path(sift, single, frames, exact, tmp_path):
    from sift_amd import cv

    img = frames[0]
    rk, rf, rd = single[exact, 0][1]
    n = len(rd)
    det = make(sift, True, exact)  # default lanes and automatic groups
    # submit / wait of 6 frames ahead: lanes, and automatic launch groups once the lanes are busy
    tickets = [det.submit(img) for _ in range(6)]
    for t in tickets:
        det.wait(t)
        k, f, d = rows(det)
        assert (k, f) == (rk, rf) and np.array_equal(d, rd), f"ticket {t}"
    # the pinned host rows the kernel writes itself
    hk, hf, hd = det.results_host()
    assert hk.tobytes() == rk and hf.tobytes() == rf and np.array_equal(hd.astype(np.float32), rd.astype(np.float32))
    # the eager masked chain
    mask = np.full((H, W), 255, np.uint8)
    mask[:, W // 2:] = 0
    k3 = np.frombuffer(rk, np.float32).reshape(-1, 3)
    keep = cv.mask_keep(k3[:, 0], k3[:, 1], mask)
    assert 0 < keep.sum() < n
    det.detectAndCompute(img, mask)
    k, f, d = rows(det)
    assert k == k3[keep].tobytes() and np.array_equal(d, rd[keep])
    # compute on the frame's own keypoints
    kp = cv.keypoint_records(k3, np.frombuffer(rf, np.float32).reshape(-1, 4))
    det.compute(img, kp)
    assert det.total_size == n and np.array_equal(rows(det)[2], rd)
    # computeDevice with one invalid keypoint: its zero row stays zero (s == 0), codes of -128, flag 16
    bad = kp.copy()
    bad["size"][3] = np.nan
    dimg, dk = sift.DeviceArray.from_numpy(img), sift.DeviceArray.from_numpy(bad)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", sift.SiftKeypointWarning)
        det.computeDevice(dimg.value, W * 4, dk.value, n)
    assert det.overflow_flags() == sift.SIFT_HIP_FLAG_BAD_KEYPOINT
    d = rows(det)[2]
    good = np.arange(n) != 3
    assert not d[3].any() and rd[3].any() and np.array_equal(d[good], rd[good])
    cp, kp_ptr = det.results_sidecar()
    codes = d2h(sift, cp, (n, 128), np.int8)
    assert np.array_equal(codes.astype(np.int32) + 128, d.astype(np.int32)) and (codes[3] == -128).all()
    keys = d2h(sift, kp_ptr, (n,), np.int32)
    c = codes.astype(np.int64)
    assert np.array_equal(keys, -(256 * (c * c).sum(axis=1) + (np.arange(n) & 255)))
    # the replay of the descriptor stage, on a dump a plain handle of the same configuration wrote
    plain = make(sift, False, exact)
    dump, out = str(tmp_path / "dump"), str(tmp_path / "out")
    plain.setDataGen(dump)
    plain.detectAndCompute(img)
    plain.setDataGen("")
    det.replayStage(dump, "descriptor", out)
    got = np.fromfile(os.path.join(out, "desc.f16"), np.float16).reshape(-1, 128).astype(np.float32)
    assert np.array_equal(got, rd.astype(np.float32))


# ---- sidecar: root rows match from their codes -------------------------------------------------------------------------
def run_match(sift, m, qp, nq, tp, nt):
    idx2, d2 = sift.DeviceArray(nq * 8), sift.DeviceArray(nq * 8)
    m.match_device(qp, nq, tp, nt, 0.8, False, idx2.value, d2.value)
    return idx2.to_numpy(np.int32, (nq, 2)), d2.to_numpy(np.float32, (nq, 2))


@pytest.fixture(scope="module")
def pair(sift, oracle, gold):
    """The crop and its rot90: the plain rows of both, and the oracle's knn-2 on their cv.rootsift bytes."""
    from sift_amd import cv

    img = gold[0]["camera256"].astype(np.float32)
    imgs = (img, np.ascontiguousarray(np.rot90(img)))
    plain = make(sift, False)
    pd = []
    for im in imgs:
        plain.detectAndCompute(im)
        pd.append(rows(plain)[2])
    ra, rb = cv.rootsift(pd[0]), cv.rootsift(pd[1])
    return imgs, (ra, rb), oracle.knn2(ra.astype(np.float32), rb.astype(np.float32))


def assert_oracle(got, knn):
    gi, gd = got
    oi, od = knn
    assert np.array_equal(gi, oi)
    assert np.array_equal(np.sqrt(gd[oi >= 0]).astype(np.float32), od[oi >= 0])


def test_sidecar_path_equals_converting_path_and_oracle(sift, pair):
    imgs, (ra, rb), knn = pair
    det = make(sift, True)
    det.detectAndCompute(imgs[0])
    det.detectAndCompute(imgs[1])
    n0, n1 = det.prev_size, det.total_size
    assert (n0, n1) == (len(ra), len(rb)) and n0 > 100
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    assert np.array_equal(device_bytes(sift, q, n0), ra) and np.array_equal(device_bytes(sift, t, n1), rb)
    m = sift.Matcher(max(n0, n1), max(n0, n1))
    side = run_match(sift, m, q, n0, t, n1)
    fq = sift.DeviceArray.from_numpy(d2h(sift, q, (n0, 128), np.uint16))
    ft = sift.DeviceArray.from_numpy(d2h(sift, t, (n1, 128), np.uint16))
    conv = run_match(sift, m, fq.value, n0, ft.value, n1)
    assert np.array_equal(side[0], conv[0]) and np.array_equal(side[1].view(np.uint32), conv[1].view(np.uint32))
    assert_oracle(side, knn)


def test_plain_buffers_transformed_in_place(sift, pair):
    """A plain detector's own buffers through rootsift_device after mutable_data(): the matcher converts the written
    rows (the stale sidecar holds the plain codes) and gives the root detector's result."""
    imgs, (ra, rb), knn = pair
    det = make(sift, False)
    det.detectAndCompute(imgs[0])
    det.detectAndCompute(imgs[1])
    n0, n1 = det.prev_size, det.total_size
    sift.rootsift_device(det.prev_descriptor.mutable_data(), n0)
    sift.rootsift_device(det.device_descriptor.mutable_data(), n1)
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    assert np.array_equal(device_bytes(sift, q, n0), ra) and np.array_equal(device_bytes(sift, t, n1), rb)
    assert_oracle(run_match(sift, sift.Matcher(max(n0, n1), max(n0, n1)), q, n0, t, n1), knn)


# ---- the stand-alone kernel ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bank():
    """4,096 fp16 rows: every byte value, 1..128 non-zero entries, the special rows of the CPU test (zero, one-hot,
    equal bytes, non-integer and non-finite inputs) and SIFT-like rows; with their cv.rootsift bytes."""
    from sift_amd import cv

    rng = np.random.default_rng(7)
    r = np.minimum(rng.exponential(30.0, (4096, 128)), 255).astype(np.uint8).astype(np.float16)  # SIFT-like
    for v in range(256):  # every byte value, on a sparse row so that large values survive
        r[v] = 0
        r[v, rng.choice(128, 8, replace=False)] = rng.integers(0, 256, 8)
        r[v, v % 128] = v
    for k in range(128):  # k + 1 non-zero entries
        r[256 + k] = 0
        r[256 + k, rng.choice(128, k + 1, replace=False)] = rng.integers(1, 256, k + 1)
    r[384] = 0
    r[385] = 0
    r[385, 5] = 200
    r[386], r[387], r[388] = 1, 7, 255
    r[389] = 0
    r[389, :7] = [0.5, 1.5, 254.5, 255.5, -3, np.nan, np.inf]
    r[390] = rng.uniform(-2, 300, 128)  # non-integers across and past the range
    r[391] = np.nan
    r[392] = -np.inf
    # rows 0, 62..64 and the last take part in the small n: keep a special one among them
    r[63] = r[389]
    want = cv.rootsift(r)
    assert want[385, 5] == 255 and (want[386:389] == 45).all() and not want[[384, 391, 392]].any()
    r.flags.writeable = False
    want.flags.writeable = False
    return r, want


FILL = 0x7777


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096])
def test_standalone_kernel(sift, bank, n):
    src, want = bank
    bits = np.ascontiguousarray(src).view(np.uint16)
    dsrc = sift.DeviceArray.from_numpy(bits)
    dout = sift.DeviceArray.from_numpy(np.full((4096, 128), FILL, np.uint16))
    sift.rootsift_device(dsrc.value, n, dout.value)
    out = dout.to_numpy(np.uint16, (4096, 128))
    assert np.array_equal(out[:n].view(np.float16).astype(np.float32), want[:n].astype(np.float32))
    assert (out[n:] == FILL).all(), "rows past n were written"
    assert np.array_equal(dsrc.to_numpy(np.uint16, (4096, 128)), bits), "the input was written"
    sift.rootsift_device(dsrc.value, n)  # in place
    out = dsrc.to_numpy(np.uint16, (4096, 128))
    assert np.array_equal(out[:n].view(np.float16).astype(np.float32), want[:n].astype(np.float32))
    assert np.array_equal(out[n:], bits[n:]), "rows past n were written"
    host = sift.rootsift(src[:n])
    assert host.dtype == np.float16 and np.array_equal(host.astype(np.float32), want[:n].astype(np.float32))


def test_standalone_kernel_two_byte_aligned_rows(sift, bank):
    """Pointers that are 2- but not 4-byte aligned (rows inside a caller's larger record): the 16-bit path."""
    src, want = bank
    n = 65
    bits = np.ascontiguousarray(src[:n]).view(np.uint16).reshape(-1)
    buf = np.full(1 + n * 128 + 3, FILL, np.uint16)
    buf[1:1 + n * 128] = bits
    dsrc = sift.DeviceArray.from_numpy(buf)
    dout = sift.DeviceArray.from_numpy(np.full(len(buf), FILL, np.uint16))
    sift.rootsift_device(dsrc.value + 2, n, dout.value + 2)
    out = dout.to_numpy(np.uint16, (len(buf),))
    assert np.array_equal(out[1:1 + n * 128].view(np.float16).astype(np.float32).reshape(n, 128), want[:n].astype(np.float32))
    assert out[0] == FILL and (out[1 + n * 128:] == FILL).all()
    sift.rootsift_device(dsrc.value + 2, n, dout.value)  # one aligned, one not
    out = dout.to_numpy(np.uint16, (len(buf),))
    assert np.array_equal(out[:n * 128].view(np.float16).astype(np.float32).reshape(n, 128), want[:n].astype(np.float32))


# ---- the default norm is today's rows ------------------------------------------------------------------------------------
def test_default_norm_is_unchanged(sift, gold):
    data, meta = gold
    img = data["camera256"].astype(np.float32)
    res = []
    for _ in range(2):
        det = sift.Detector(config_for(sift, meta["configs"]["default"]))  # never calls the setter
        assert not det.root_sift
        det.gpuWarmUpAndAllocate()
        det.detectAndCompute(img)
        res.append(gpu_keypoints(det))
    (gk, gd, _), (gk2, gd2, _) = res
    assert gk.tobytes() == gk2.tobytes() and np.array_equal(gd, gd2)
    ok, od = data["default_kpts"], data["default_desc"].astype(np.float32)
    assert_same_keypoints(gk, ok)
    assert_descriptor_bar(gd[sort_keys(gk)], od[sort_keys(ok)], "golden, default norm")
