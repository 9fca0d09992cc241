"""trace tcp's per-row rules (csrc/k_tcptrace.h, the function the device kernel runs) on the CPU
under AddressSanitizer + UndefinedBehaviorSanitizer: tests/sanitize/tcptrace_main.cpp, a stand-alone
program, runs it over the exhaustive small field table (every probe, three families, every field
zero or not in each position, six filter settings) against a second restatement written the way the
BPF programs are.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_classify_row_under_asan_ubsan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (set CXX)")
    exe = str(tmp_path / "tcptrace_main")
    # gcc links the sanitizer runtimes dynamically unless told otherwise (clang links them in)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", *static, "-I", os.path.join(ROOT, "inspektor-gadget_amd", "csrc"),
                        os.path.join(HERE, "sanitize", "tcptrace_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "TCP_OK rows=4608" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
