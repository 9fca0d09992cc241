"""traceloop's shared host/device core (csrc/k_traceloop.h) on the CPU under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/sanitize/traceloop_main.cpp, a stand-alone program, runs the
join's keys, codes, summary operator (cut into random tiles, combined under random
parenthesisations) and class rule the way the device does and compares the events with
Tracer.Read's maps and loops restated row by row, on the hand-worked groups, random colliding
streams and single groups of thousands of rows.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_summary_equals_maps_under_asan_ubsan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler (set CXX)")
    exe = str(tmp_path / "traceloop_main")
    # gcc links the sanitizer runtimes dynamically unless told otherwise (clang links them in)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", *static, "-I", os.path.join(ROOT, "inspektor-gadget_amd", "csrc"),
                        os.path.join(HERE, "sanitize", "traceloop_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "TL_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
