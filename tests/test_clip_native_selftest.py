"""SlotTable::wait_comm / epilogue_stream (csrc/comm/slot_table.h), the host logic a clip group's commit adds to the
request-slot state machine, under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program
(tests/native/wait_comm_selftest.cpp) against a simulated device with random stream interleavings, in every engine
mode."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_wait_comm_selftest_asan_ubsan(tmp_path):
    exe = tmp_path / "wait_comm_selftest"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tests", "native", "wait_comm_selftest.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")  # (the options of tests/test_native_sanitizers.py)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK")
    assert "runtime error" not in r.stderr
