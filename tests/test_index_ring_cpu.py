"""csrc/index_ring.h: the arithmetic of the sampled training loop's index storage -- where member m's indices and batch size
of an iteration lie on the host and on the device, which chunks are uploaded and which host slots go back to the samplers, and
where the iteration after a given one is found.  Host code only: tests/native/index_ring_check.cpp, a stand-alone program, is
built with g++ -fsanitize=address,undefined and once more plainly, and run here, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "index_ring_check.cpp")
INC = os.path.join(ROOT, "graph-neural-net_amd", "csrc")


@pytest.mark.parametrize("sanitize", [True, False])
def test_layout_window_and_successor(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path / "index_ring_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I", INC] + flags + ["-o", out, SRC], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "index ring ok"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
