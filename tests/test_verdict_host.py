"""The fast round's status ladder and reliability arithmetic (csrc/include/svoc/verdict.hpp: the code all five fast
kernels and the CPU twin call) against tables written out in csrc/selftest/verdict_selftest.cpp: R = 0 .. 5, both
contracts, both forms, reliabilities just inside, on and outside 0 and 1, NaN, max_spread = 0.  A stand-alone program
built here with the address and undefined-behaviour sanitizers and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_verdict_selftest_under_sanitizers(tmp_path):
    exe = str(tmp_path / "verdict_selftest")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I" + os.path.join(ROOT, "csrc", "include"), os.path.join(ROOT, "csrc", "selftest", "verdict_selftest.cpp"),
         "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
    assert "verdict_selftest: ok" in run.stdout
