"""The count the launch-alone programs' guard and margin checks all go through (changed_outside, tests/cpp/check_common.hpp), without a GPU:
tests/cpp/changed_outside_test.cpp on host arrays - a clean buffer, one changed element at each end of each margin, the first and last logical
element (not counted), a zero-length logical range, a front-only layout."""
import subprocess

from launch_harness import build


def test_changed_outside_counts_the_margins_and_only_them(tmp_path):
    out = subprocess.run([build(tmp_path, "changed_outside_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout + out.stderr
