"""The track record's scalar arithmetic (csrc/include/svoc/track.hpp: the exact score against wsad.hpp's i128
wsad_div at its edges, the fast score, track_update_one) as exact integers: csrc/selftest/track_selftest.cpp, a
stand-alone program built here with the address and undefined-behaviour sanitizers and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_track_selftest_under_sanitizers(tmp_path):
    exe = str(tmp_path / "track_selftest")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I" + os.path.join(ROOT, "csrc", "include"), os.path.join(ROOT, "csrc", "selftest", "track_selftest.cpp"),
         "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert run.returncode == 0, run.stdout
    assert "track_selftest: ok" in run.stdout
