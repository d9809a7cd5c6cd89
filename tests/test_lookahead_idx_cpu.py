"""csrc/lookahead.h, the index-range form of Lookahead::rebased: in a group call with one sampler per member, member k's index
pointers lie k * idx_S behind member 0's inside the device index region.  Host code only: tests/native/lookahead_idx_check.cpp,
a stand-alone program, is built with g++ and run here, no GPU -- with -fsanitize=address,undefined, and once more plainly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lookahead_idx_check.cpp")


@pytest.mark.parametrize("sanitize", [True, False])
def test_lookahead_index_region(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path / "lookahead_idx_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", out, SRC], check=True, capture_output=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "lookahead idx ok"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
