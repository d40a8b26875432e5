"""The host-side rules that need no device, checked by stand-alone programs under the host sanitizers: those of the C ABI
(grl_amd/csrc/grlx_host_rules.h: what a projector admits -- finite, |x * scaling| < 2^30 --, table growth, the stream distance of the initial parameters, the byte counts of tables, target values
and traces; tools/host_rules_check.cpp) and those of the host layer above it (grl_amd/csrc/host/report_rules.h: file names, row texts,
the simple regret, row caps and the statistics of the report files; tools/host_report_check.cpp).  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tools", "host_rules_check.cpp")
REPORT_CHECK = os.path.join(ROOT, "tools", "host_report_check.cpp")


def _build_and_run(source, tmp_path, ok):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build " + os.path.relpath(source, ROOT))
    exe = str(tmp_path / os.path.splitext(os.path.basename(source))[0])
    res = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          source, "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert ok in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stdout + res.stderr


def test_host_rules_hold_their_stated_properties_under_the_host_sanitizers(tmp_path):
    _build_and_run(CHECK, tmp_path, "host rules ok")


def test_host_report_rules_give_their_literal_values_under_the_host_sanitizers(tmp_path):
    _build_and_run(REPORT_CHECK, tmp_path, "host report rules ok")
