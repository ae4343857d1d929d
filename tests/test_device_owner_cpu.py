"""csrc/device_owner.h on the CPU: the header every handle of the library owns its device memory, streams and events through, compiled
against a fake backend (tests/device_owner_test.cpp) that counts live objects and fails the k-th malloc / memset -- what cannot be
provoked on a GPU.  A stand-alone program built with g++ -fsanitize=address,undefined and run directly (no preload): a double free, a
use after free of the fake's heap blocks fails the run as well as the program's own checks do (which count what is left alive).
The sanitizer runtime is linked statically, so the program does not care what else the process environment preloads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["destructor", "malloc_failure", "memset_failure", "release", "release_foreign", "zero_bytes", "destruction_order", "temp", "regrow"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    asan = subprocess.run(["gcc", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip() if gxx else ""
    if not gxx or not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("g++ / libasan not available")
    exe = str(tmp_path_factory.mktemp("device_owner") / "device_owner_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "concepthash_amd", "csrc"), os.path.join(ROOT, "tests", "device_owner_test.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("case", CASES)
def test_device_owner(program, case):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program, case], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {case}", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
