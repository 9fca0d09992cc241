"""profile cpu's shared host/device core (csrc/k_stack.h) on the CPU under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/sanitize/stack_main.cpp, a stand-alone program, checks the
symbol search against a second implementation on random sorted and unsorted tables of 0 to 1000
symbols, and the row hash over every row_bytes from 8 to 1024 on buffers that end exactly at the
row.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_search_and_hash_under_asan_ubsan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (set CXX)")
    exe = str(tmp_path / "stack_main")
    # gcc links the sanitizer runtimes dynamically unless told otherwise (clang links them in)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", *static, "-I", os.path.join(ROOT, "inspektor-gadget_amd", "csrc"),
                        os.path.join(HERE, "sanitize", "stack_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ST_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
