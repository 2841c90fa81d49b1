"""CPU tier of the buffer owner (csrc/device_buffer.h): the template over a counting fake allocator, as a stand-alone program
under the host sanitizers. Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_owner_under_asan_ubsan(tmp_path):
    """alloc / ensure / replace / borrow / move of csrc/device_buffer.h (plain C++, no HIP) compiled on their own with
    -fsanitize=address,undefined by tests/sanitize/buffer_sanitize.cpp: sizes and the account, the order of free and
    allocation, failures half way, error codes and texts, for a device-like and a pinned-like policy; the fake aborts on a
    double free, and at exit nothing is live"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "buffer_sanitize"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), os.path.join(ROOT, "tests", "sanitize", "buffer_sanitize.cpp")], check=True, timeout=600)
    pr = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, TMPDIR=str(tmp_path), UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert pr.returncode == 0 and "buffer_sanitize ok" in pr.stdout, (pr.stdout[-2000:], pr.stderr[-3000:])
    assert "runtime error" not in pr.stderr and "AddressSanitizer" not in pr.stderr and "LeakSanitizer" not in pr.stderr
