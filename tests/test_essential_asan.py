"""Host code of the essential surface (csrc/verify_cxx.cpp: the batched methods' camera rule, and the argument rules of
the C ABI of sift_hip_verifier_reserve_essential / sift_hip_verify_essential_* under it) under
-fsanitize=address,undefined: `make asan` links it into the stand-alone CPU program tests/cpp/test_essential_args.cpp
(argument validation; no GPU needed), the way tests/test_affine_asan.py runs tests/cpp/test_affine_args.cpp.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_ENV = {"ASAN_OPTIONS": "abort_on_error=0:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_essential_arguments_under_asan():
    exe = os.path.join(ROOT, "another-cuda-sift_amd", "lib", "asan", "test_essential_args")
    r = subprocess.run(["make", "-C", ROOT, exe.replace(ROOT + os.sep, "")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    syms = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_" in syms and "__ubsan_" in syms, "not a sanitizer build"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ASAN_ENV))
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "essential args ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
