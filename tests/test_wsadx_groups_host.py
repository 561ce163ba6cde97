"""The R <= 256 arithmetic of the wide-column exact kernel's lane-group form (csrc/include/svoc/wsad_wide.hpp:
var_floor_g, zpow_g, skew_kurt_g, and the row-count-independent routines at the values 256 rows reach) against the
i128 routines of wsad.hpp, as exact integers: csrc/selftest/wsadx_groups_selftest.cpp, a stand-alone program built
here with the address and undefined-behaviour sanitizers and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_wsadx_groups_selftest_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wsadx_groups_selftest")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I" + os.path.join(ROOT, "csrc", "include"), os.path.join(ROOT, "csrc", "selftest", "wsadx_groups_selftest.cpp"),
         "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert run.returncode == 0, run.stdout
    assert "wsadx_groups_selftest: ok" in run.stdout
