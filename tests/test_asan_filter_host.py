"""CPU: the filtered host BM25 (cbv2_bm25_search_filtered) built with
-fsanitize=address,undefined by g++ and driven by the stand-alone program
tests/asan/asan_filter_driver.cpp (partial last bitmap words, empty and full
filters, k above the allowed count).  The sanitizer runs in that program only;
no GPU code is instrumented."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-rag-colbertv2_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_filtered_bm25_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "asan_filter_driver")
    srcs = [os.path.join(ROOT, "tests", "asan", "asan_filter_driver.cpp"), os.path.join(CSRC, "host_bm25.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), *srcs, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "0 failed checks" in r.stdout
