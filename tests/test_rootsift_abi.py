"""sift_hip_set_descriptor_norm / sift_hip_rootsift_*: the host-side logic that runs before any device call
(host-only handles, as tests/test_abi.py::test_descriptor_mode_host_logic).  CPU only."""
import ctypes

import pytest

INVALID, STATE = -1, -3  # SIFT_HIP_ERR_INVALID, SIFT_HIP_ERR_STATE


@pytest.fixture()
def handle(sift):
    L = sift.lib()
    h = ctypes.c_void_p()
    c = sift._Config()
    L.sift_hip_default_config(ctypes.byref(c), 64, 64)
    assert L.sift_hip_create(ctypes.byref(c), 0, ctypes.byref(h)) == 0
    yield L, h
    L.sift_hip_destroy(h)


def test_norm_constants(sift):
    assert (sift.SIFT_HIP_NORM_L2, sift.SIFT_HIP_NORM_ROOT) == (0, 1)


def test_norm_get_set(sift, handle):
    L, h = handle
    n = ctypes.c_int(-1)
    assert L.sift_hip_descriptor_norm(h, ctypes.byref(n)) == 0 and n.value == sift.SIFT_HIP_NORM_L2
    assert L.sift_hip_set_descriptor_norm(h, 2) == INVALID and b"norm" in L.sift_hip_last_error()
    assert L.sift_hip_set_descriptor_norm(h, -1) == INVALID
    assert L.sift_hip_descriptor_norm(h, ctypes.byref(n)) == 0 and n.value == sift.SIFT_HIP_NORM_L2
    assert L.sift_hip_set_descriptor_norm(h, sift.SIFT_HIP_NORM_ROOT) == 0
    assert L.sift_hip_descriptor_norm(h, ctypes.byref(n)) == 0 and n.value == sift.SIFT_HIP_NORM_ROOT
    # independent of the descriptor mode: all four combinations
    m = ctypes.c_int(-1)
    for mode in (sift.SIFT_HIP_DESC_EXACT, sift.SIFT_HIP_DESC_FAST):
        for norm in (sift.SIFT_HIP_NORM_L2, sift.SIFT_HIP_NORM_ROOT):
            assert L.sift_hip_set_descriptor_mode(h, mode) == 0 and L.sift_hip_set_descriptor_norm(h, norm) == 0
            assert L.sift_hip_descriptor_mode(h, ctypes.byref(m)) == 0 and m.value == mode
            assert L.sift_hip_descriptor_norm(h, ctypes.byref(n)) == 0 and n.value == norm
    assert L.sift_hip_descriptor_norm(h, None) == INVALID


def test_null_handle(sift):
    L = sift.lib()
    n = ctypes.c_int()
    assert L.sift_hip_set_descriptor_norm(None, sift.SIFT_HIP_NORM_ROOT) == INVALID
    assert L.sift_hip_descriptor_norm(None, ctypes.byref(n)) == INVALID


def test_datagen_and_root_exclude_each_other(sift, handle, tmp_path):
    L, h = handle
    assert L.sift_hip_set_descriptor_norm(h, sift.SIFT_HIP_NORM_ROOT) == 0
    assert L.sift_hip_set_datagen(h, str(tmp_path).encode()) == STATE
    assert b"ROOT" in L.sift_hip_last_error()
    assert L.sift_hip_set_datagen(h, b"") == 0 and L.sift_hip_set_datagen(h, None) == 0  # switching off is no dump
    assert L.sift_hip_set_descriptor_norm(h, sift.SIFT_HIP_NORM_L2) == 0
    assert L.sift_hip_set_datagen(h, str(tmp_path).encode()) == 0
    assert L.sift_hip_set_descriptor_norm(h, sift.SIFT_HIP_NORM_ROOT) == STATE
    assert b"ROOT" in L.sift_hip_last_error() and b"datagen" in L.sift_hip_last_error()
    n = ctypes.c_int(-1)
    assert L.sift_hip_descriptor_norm(h, ctypes.byref(n)) == 0 and n.value == sift.SIFT_HIP_NORM_L2
    assert L.sift_hip_set_descriptor_norm(h, sift.SIFT_HIP_NORM_L2) == 0  # L2 with dumps on stays valid
    assert L.sift_hip_set_datagen(h, None) == 0
    assert L.sift_hip_set_descriptor_norm(h, sift.SIFT_HIP_NORM_ROOT) == 0


def test_python_surface(sift):
    d = sift.Detector(sift.CudaSiftConfig(col_width=64, row_width=64), device=0, root_sift=True)
    n = ctypes.c_int(-1)
    assert d.root_sift and not d.exact_descriptors
    assert sift.lib().sift_hip_descriptor_norm(d.handle, ctypes.byref(n)) == 0 and n.value == sift.SIFT_HIP_NORM_ROOT
    with pytest.raises(sift.SiftHipError, match="ROOT"):
        d.setDataGen("/tmp/never-written")
    assert not sift.Detector(sift.CudaSiftConfig(col_width=64, row_width=64), device=0).root_sift


@pytest.mark.parametrize("fn", ["sift_hip_rootsift_device", "sift_hip_rootsift_host"])
def test_transform_argument_refusals(sift, fn):
    """Refused before any device call: the pointers are never read."""
    L = sift.lib()
    f = getattr(L, fn)
    call = (lambda i, n, o: f(i, n, o, None)) if fn.endswith("device") else f
    A = 0x10000000  # 256-byte aligned addresses, never dereferenced
    assert call(A, -1, A + 0x100000) == INVALID and b"negative" in L.sift_hip_last_error()
    assert call(None, 4, A) == INVALID and call(A, 4, None) == INVALID and call(None, 1, None) == INVALID
    assert call(A + 1, 4, A + 0x100000) == INVALID and call(A, 4, A + 0x100001) == INVALID  # odd pointers
    assert call(A + 1, 4, A + 1) == INVALID
    for off in (2, 256, 4 * 256 - 2):  # partial overlap of the 4 * 256-byte ranges, either order
        assert call(A, 4, A + off) == INVALID and b"overlap" in L.sift_hip_last_error(), off
        assert call(A + off, 4, A) == INVALID, off
    # n == 0 is a no-op whatever the pointers
    assert call(None, 0, None) == 0 and call(A + 1, 0, A + 3) == 0 and call(A, 0, A + 2) == 0


def test_python_transform_refusals(sift):
    with pytest.raises(sift.SiftHipError, match="negative"):
        sift.rootsift_device(0x10000000, -1)
    with pytest.raises(sift.SiftHipError, match="overlap"):
        sift.rootsift_device(0x10000000, 2, 0x10000100)
    import numpy as np

    with pytest.raises(ValueError):
        sift.rootsift(np.zeros((3, 64), np.float16))
    assert sift.rootsift(np.zeros((0, 128), np.float16)).shape == (0, 128)
