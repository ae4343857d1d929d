"""csrc/layer_forward.h on the CPU: the one definition of the LN-folded encoder layer's launch sequence, which ch_encode and the training
step both issue, compiled against a launcher that records every call (tests/layer_forward_test.cpp) and compared, field by field -- call
kind, rows, epilogue, extents, every pointer and leading dimension -- with the sequences of the two hand-written chains it replaced.  A
changed epilogue choice or a swapped buffer shows here without a GPU; the GPU suite's tolerances would not show the former.
A stand-alone program built with g++ -fsanitize=address,undefined and run directly (no preload), the sanitizer runtime linked statically."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# encode: layer 0 (plain qkv on pre-normalised rows), a middle layer (folded qkv), the last layer pruning / not pruning (no statistics
# from the last up-projection); training: a middle layer (per-layer buffers, two-output epilogues), the pruning last layer (statistics
# into the dummies); act = 1 (erf-GELU fc1) in both
CASES = ["encode_layer0", "encode_middle", "encode_last_pruned", "encode_last", "train_middle", "train_last_pruned", "encode_gelu", "train_gelu"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    asan = subprocess.run(["gcc", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip() if gxx else ""
    if not gxx or not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("g++ / libasan not available")
    exe = str(tmp_path_factory.mktemp("layer_forward") / "layer_forward_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "concepthash_amd", "csrc"), os.path.join(ROOT, "tests", "layer_forward_test.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("case", CASES)
def test_layer_forward(program, case):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program, case], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {case}", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
