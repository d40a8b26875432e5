"""The host-side rules of the C ABI that need no device (grl_amd/csrc/grlx_host_rules.h: table growth, the stream distance of the initial
parameters, the byte counts of tables, target values and traces), checked by a stand-alone program under the host sanitizers
(tools/host_rules_check.cpp).  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tools", "host_rules_check.cpp")


def test_host_rules_hold_their_stated_properties_under_the_host_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/host_rules_check.cpp")
    exe = str(tmp_path / "host_rules_check")
    res = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          CHECK, "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host rules ok" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stdout + res.stderr
