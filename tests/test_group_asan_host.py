"""CPU: csrc/groups_host.cpp (cbv2_groups_build_host, the host half of a
grouping) built with -fsanitize=address,undefined by g++ into a stand-alone
program (tests/asan/groups_driver.cpp) that calls it with output arrays of
exactly the documented sizes.  Host code only: nothing here touches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_groups_host_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "groups_driver")
    srcs = [os.path.join(ROOT, "tests", "asan", "groups_driver.cpp"),
            os.path.join(ROOT, "hybrid-rag-colbertv2_amd", "csrc", "groups_host.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), *srcs, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failed checks" in r.stdout
