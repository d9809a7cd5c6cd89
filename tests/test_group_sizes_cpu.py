"""csrc/group_sizes.h: the per-iteration decision of a group call with one batch size per member (every member's live rows now and
in the announced iteration; whether the announced batch has the current batch's size for EVERY member) and the group's record of
member k's sizes under member 0's look-ahead state.  Host code only: tests/native/group_sizes_check.cpp, a stand-alone program,
is built with g++ and run here, no GPU -- with -fsanitize=address,undefined, and once more plainly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "group_sizes_check.cpp")


@pytest.mark.parametrize("sanitize", [True, False])
def test_group_sizes_transitions(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path / "group_sizes_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", out, SRC], check=True, capture_output=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "group sizes ok"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
